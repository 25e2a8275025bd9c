"""Batches for the GPU tests of one-pass RX reassembly: frames placed in an arena, the canaried
output arena, and the model's result (tests/rxr_model.py) for one placement. Test infrastructure only."""
import functools
import importlib.util
import os
import re

import numpy as np

import nstack_amd as na
import rxr_model as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSET = 0xCCCCCCCC
# the frame builders of the golden generator (ip_packet, frame, fragments)
_spec = importlib.util.spec_from_file_location("make_rxr_golden", os.path.join(ROOT, "tests", "golden", "make_rxr_golden.py"))
mg = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mg)
PLAN_KEYS = ("fstat", "dst", "dgi", "doff", "dlen", "dlead")


@functools.lru_cache(maxsize=None)
def _classify(f, flags, dropped):
    return rr.classify(f, flags, dropped)


def classify_fn(f, flags, dropped):
    """rr.classify, memoised on the frame without its ip_id (scale batches restamp the id of a small
    pool of frames): the id only names the group."""
    if len(f) < 34:
        return _classify(f, flags, dropped)
    c = _classify(f[:18] + b"\x00\x00" + f[20:], flags, dropped)
    return c if c[6] is None else c[:6] + ((c[6][0], c[6][1], int.from_bytes(f[18:20], "big")),)


def to_dev(arr, dev):
    import torch
    arr = np.ascontiguousarray(arr)
    return torch.from_numpy(arr if arr.flags.writeable else arr.copy()).to(dev)


def engine_constants():
    """The host pipeline's chunk bounds, read from rxr_engine.cpp: {name: value}."""
    with open(os.path.join(ROOT, "nstack_amd", "csrc", "rxr_engine.cpp")) as f:
        src = f.read()
    k = {m[0]: int(m[1]) << int(m[2]) for m in re.findall(r"constexpr uint64_t (k\w+) = (\d+)ull << (\d+);", src)}
    assert set(k) == {"kInBytes", "kOutBytes", "kChunkDgs", "kChunkFrames"}, k
    return k


def host_chunks(pl, k=None):
    """The chunks run_host (rxr_engine.cpp) forms from a plan: [(k0, k1, frames, bound)], datagrams
    [k0, k1), with `bound` the condition that refused datagram k1: "dgs", "frames", "in", "out", or
    "end" for the last chunk."""
    k = k or engine_constants()
    m = pl["m"]
    nfr, gsum = np.zeros(m, dtype=np.int64), np.zeros(m, dtype=np.int64)
    for i, c in enumerate(pl["cls"]):
        if pl["dgi"][i] != rr.NONE32:
            nfr[int(pl["dgi"][i])] += 1
            gsum[int(pl["dgi"][i])] += 14 + c[2]
    doff, dlen = pl["doff"].astype(np.int64), pl["dlen"].astype(np.int64)
    out, k0 = [], 0
    while k0 < m:
        e, frames, inb, bound = k0, 0, 0, "end"
        while e < m:
            if e - k0 >= k["kChunkDgs"]:
                bound = "dgs"
            elif frames + nfr[e] > k["kChunkFrames"]:
                bound = "frames"
            elif inb + gsum[e] > k["kInBytes"]:
                bound = "in"
            elif doff[e] + dlen[e] - doff[k0] > k["kOutBytes"]:
                bound = "out"
            else:
                frames, inb, e = frames + nfr[e], inb + gsum[e], e + 1
                continue
            break
        assert e > k0
        out.append((k0, e, int(frames), bound))
        k0 = e
    return out


class RBatch:
    """A batch of frames and the model's result for one placement. `frames` is a list of frames laid
    out by rr.layout (lead, gap, order), or `placed` = (arena, off, len) is taken as it is. front/back:
    that many random bytes lie around the declared arena in the device tensor. out_base sets the
    alignment of `out` (mod 16); out_bytes = None gives exactly the room the plan asks for."""

    def __init__(self, inet_oracle, frames=None, flags=0, verdict=None, drop_mask=0, align=1, lead=0, gap=0, order=None,
                 out_base=0, out_bytes=None, seed=1, placed=None, front=0, back=0):
        self.flags, self.drop_mask, self.align = flags, drop_mask, align
        if placed is None:
            self.arena, self.off, self.ln = rr.layout(frames, lead=lead, gap=gap, order=order)
            if not frames:
                self.arena = self.arena[:lead]
        else:
            self.arena = np.ascontiguousarray(placed[0], dtype=np.uint8)
            self.off, self.ln = np.asarray(placed[1], dtype=np.uint64), np.asarray(placed[2], dtype=np.uint32)
            buf = self.arena.tobytes()
            # a frame that does not lie inside the arena is a frame of no bytes to the device plan
            frames = [buf[int(o):int(o) + int(d)] if int(o) + int(d) <= len(buf) else b"" for o, d in zip(self.off, self.ln)]
        self.frames, self.n = frames, len(frames)
        self.verdict = None if verdict is None else np.asarray(verdict, dtype=np.uint32)
        self.plan = rr.plan(frames, flags, self.verdict, drop_mask, align, classify_fn)
        self.m = self.plan["m"]
        self.need = int(self.plan["doff"][self.m - 1]) + int(self.plan["dlen"][self.m - 1]) if self.m else 0
        self.out_bytes = self.need if out_bytes is None else out_bytes
        self.base = 64 + out_base                  # canary bytes in front of `out`
        rng = np.random.default_rng(seed + 7)
        self.out0 = rng.integers(0, 256, self.base + max(self.out_bytes, int(self.plan["doff"][self.m])) + 64, dtype=np.uint8)
        body, self.fstat = rr.build(inet_oracle, frames, self.plan, self.out0[self.base:], self.out_bytes)
        self.expect = self.out0.copy()
        self.expect[self.base:] = body
        self.front = front
        self.around = np.concatenate([rng.integers(0, 256, front, dtype=np.uint8), self.arena,
                                      rng.integers(0, 256, back, dtype=np.uint8)]) if front or back else self.arena

    # ---- the device forms ----
    def launch_dev(self, dev, stream=None, dlead=True, counts=True, fstat=True, inplace=False):
        """plan_dev + reasm_dev, not waited for: the device tensors, for collect() after a synchronise."""
        import torch
        n1 = max(self.n, 1)
        d_arena = to_dev(self.around if self.around.size else np.zeros(1, np.uint8), dev)
        d_off, d_ln = to_dev(self.off if self.n else np.zeros(1, np.uint64), dev), to_dev(self.ln if self.n else np.zeros(1, np.uint32), dev)
        d_v = None if self.verdict is None else to_dev(self.verdict, dev)
        fa = d_arena.data_ptr() + self.front
        t = dict(fstat=torch.full((n1,), -1, dtype=torch.int32, device=dev),
                 dst=torch.full((n1,), 0x5555555555555555, dtype=torch.int64, device=dev),
                 dgi=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 doff=torch.full((self.n + 1,), 0x5555555555555555, dtype=torch.int64, device=dev),
                 dlen=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 dlead=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 counts=torch.full((2,), 0x5555555555555555, dtype=torch.int64, device=dev),
                 final=torch.full((n1,), -1, dtype=torch.int32, device=dev), out=to_dev(self.out0, dev))
        na.rx_reasm_plan_dev(fa, self.arena.size, d_off, d_ln, self.n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"],
                             t["dlead"] if dlead else None, t["counts"] if counts else None, flags=self.flags, verdict=d_v,
                             drop_mask=self.drop_mask, align=self.align, stream=stream)
        t["pstat"] = t["fstat"].clone() if inplace else t["fstat"]
        na.rx_reasm_dev(fa, self.arena.size, d_off, d_ln, self.n, t["pstat"], t["dst"], t["dgi"], t["doff"], t["dlen"],
                        t["out"].data_ptr() + self.base, self.out_bytes, flags=self.flags,
                        fstat=(t["pstat"] if inplace else t["final"]) if fstat else None, stream=stream)
        if inplace:
            t["final"] = t["pstat"]
        t["keep"] = (d_arena, d_off, d_ln, d_v)
        return t

    def run_dev(self, dev, stream=None, **kw):
        import torch
        if stream is not None:   # the tensors are made and filled on the stream the library works on
            with torch.cuda.stream(stream):
                t = self.launch_dev(dev, stream, **kw)
            stream.synchronize()
        else:
            t = self.launch_dev(dev, None, **kw)
            torch.cuda.synchronize()
        return self.collect(t)

    def collect(self, t):
        u = {"fstat": np.uint32, "dst": np.uint64, "dgi": np.uint32, "doff": np.uint64, "dlen": np.uint32, "dlead": np.uint32,
             "counts": np.uint64, "final": np.uint32, "out": np.uint8}
        return {k: t[k].cpu().numpy().view(v) for k, v in u.items()}

    def check_plan(self, r, dlead=True, counts=True):
        m = self.m
        assert np.array_equal(r["fstat"][:self.n], self.plan["fstat"]), ("fstat", r["fstat"][:8], self.plan["fstat"][:8])
        for k in ("dst", "dgi"):
            assert np.array_equal(r[k][:self.n], self.plan[k]), k
        assert np.array_equal(r["doff"][:m + 1], self.plan["doff"]), "doff"
        assert np.array_equal(r["dlen"][:m], self.plan["dlen"]), "dlen"
        if dlead:
            assert np.array_equal(r["dlead"][:m], self.plan["dlead"]), "dlead"
        else:
            assert (r["dlead"] == 0x55555555).all()
        if counts:
            assert r["counts"].tolist() == [m, int(self.plan["doff"][m])]
        else:
            assert (r["counts"] == 0x5555555555555555).all()

    def check_dev(self, r, fstat=True, **kw):
        self.check_plan(r, **kw)
        diff = np.flatnonzero(r["out"] != self.expect)
        assert diff.size == 0, ("device form", diff[:8] - self.base, self.plan["doff"][:4])
        if fstat:
            assert np.array_equal(r["final"][:self.n], self.fstat), ("final", r["final"][:8], self.fstat[:8])
        else:
            assert (r["final"] == 0xFFFFFFFF).all()

    # ---- the host form ----
    def run_host(self):
        out = self.out0.copy()
        n1 = max(self.n, 1)
        o = dict(fstat=np.full(n1, 0xFFFFFFFF, np.uint32), doff=np.full(self.n + 1, UNSET, np.uint64),
                 dlen=np.full(n1, UNSET, np.uint32), dlead=np.full(n1, UNSET, np.uint32))
        m = na.rx_reasm_host(self.arena, self.arena.size, self.off, self.ln, self.n, out[self.base:], self.out_bytes,
                             flags=self.flags, verdict=self.verdict, drop_mask=self.drop_mask, align=self.align, **o)
        return out, o, m

    def check_host(self):
        out, o, m = self.run_host()
        assert m == self.m
        self.host_cut = na.rxr_last_host_chunks()                         # what the engine itself cut
        diff = np.flatnonzero(out != self.expect)
        assert diff.size == 0, ("host form", diff[:8] - self.base)
        assert np.array_equal(o["fstat"][:self.n], self.fstat)
        assert np.array_equal(o["doff"][:m + 1], self.plan["doff"]) and np.array_equal(o["dlen"][:m], self.plan["dlen"])
        assert np.array_equal(o["dlead"][:m], self.plan["dlead"])

    def check(self, dev, host=True):
        self.check_dev(self.run_dev(dev))
        if host and self.out_bytes >= self.need:
            self.check_host()
