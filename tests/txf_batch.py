"""Batches for the GPU tests of one-pass TX framing: datagrams placed in an arena, the canaried
output arena, and the model's result (tests/txf_model.py) for one placement. A batch is made from a
list of datagrams (`pack` places them) or from an arena with off[] and len[] as they are, so that
off[] may point many times into a small pool. Test infrastructure only."""
import functools
import os
import re

import numpy as np

import nstack_amd as na
import txf_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FCS = fm.F_FCS
UNSET = 0xCCCCCCCC

_ORACLES = {}


@functools.lru_cache(maxsize=None)
def _frames(dg, mac, mtu, flags):
    return fm.frames(_ORACLES["fcs"], _ORACLES["inet"], dg, mac, mtu, flags)


def frames_fn(fcs_oracle, inet_oracle, dg, mac, mtu, flags):
    """fm.frames, memoised: the frames of a datagram do not depend on where they are placed."""
    _ORACLES["fcs"], _ORACLES["inet"] = fcs_oracle, inet_oracle
    return _frames(bytes(dg), bytes(mac), mtu, flags)


def to_dev(arr, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def datagram(rng, hlen, B, foff=0, vhl=None, ip_len=None, proto=253):
    """An IPv4 datagram of random bytes: options, payload and the checksum field are garbage."""
    D = hlen + B
    b = bytearray(rng.integers(0, 256, D, dtype=np.uint8).tobytes())
    b[0] = (0x40 | hlen // 4) if vhl is None else vhl
    b[2:4] = int(D if ip_len is None else ip_len).to_bytes(2, "big")
    b[6:8] = int(foff).to_bytes(2, "big")
    b[9] = proto
    return bytes(b)


def pack(dgs, seed=1, aligns=None):
    """Datagrams into one arena of random bytes, datagram i at aligns[i] mod 4 (random by default)."""
    rng = np.random.default_rng(seed)
    arena = rng.integers(0, 256, sum(len(d) + 8 for d in dgs) + 16, dtype=np.uint8)
    off, pos = [], 0
    for i, d in enumerate(dgs):
        a = int(rng.integers(0, 4)) if aligns is None else aligns[i]
        pos += (a - pos) % 4
        off.append(pos)
        arena[pos:pos + len(d)] = np.frombuffer(d, dtype=np.uint8)
        pos += len(d) + int(rng.integers(0, 4))
    return arena[:pos].copy(), np.array(off, dtype=np.uint64), np.array([len(d) for d in dgs], dtype=np.uint32)


def macs_of(n, seed=2):
    return np.random.default_rng(seed).integers(0, 256, (n, 12), dtype=np.uint8)


def engine_constants():
    """The host pipeline's chunk bounds, read from txf_engine.cpp: {name: value}."""
    with open(os.path.join(ROOT, "nstack_amd", "csrc", "txf_engine.cpp")) as f:
        src = f.read()
    k = {m[0]: int(m[1]) << int(m[2]) for m in re.findall(r"constexpr uint64_t (k\w+) = (\d+)ull << (\d+);", src)}
    assert set(k) == {"kInBytes", "kOutBytes", "kChunkDgs", "kChunkFrames"}, k
    return k


def host_chunks(first, ln, slot, k=None):
    """The chunks run_host (txf_engine.cpp) forms from a host plan: [(i, e, frames, bound)], datagrams
    [i, e), with `bound` the condition that refused datagram e: "dgs", "in", "frames", "out", or "end"
    for the last chunk. The four conditions are monotone in e, so the loop's e is their minimum."""
    k = k or engine_constants()
    first = np.asarray(first, dtype=np.uint64).astype(np.int64)
    n = first.size - 1
    glen = np.where(first[1:] > first[:-1], np.asarray(ln, dtype=np.int64), 0)
    cs = np.concatenate([[0], np.cumsum(glen)])
    out, i = [], 0
    while i < n:
        lim = {"end": n, "dgs": i + k["kChunkDgs"],      # the loop's order of conditions: the first that fails
               "in": int(np.searchsorted(cs, cs[i] + k["kInBytes"], "right")) - 1,
               "frames": int(np.searchsorted(first, first[i] + k["kChunkFrames"], "right")) - 1,
               "out": int(np.searchsorted(first, first[i] + k["kOutBytes"] // slot, "right")) - 1}
        bound = min(lim, key=lambda b: lim[b])
        e = lim[bound]
        assert e > i
        out.append((i, e, int(first[e] - first[i]), bound))
        i = e
    return out


class Batch:
    """A batch and the model's result for one placement. `dgs` is a list of datagrams to pack, or
    `placed` = (arena, off, len) is taken as it is. front/back: that many random bytes lie around the
    declared arena in the device tensor, so `dgram` is the tensor's base + front."""

    def __init__(self, oracle, inet_oracle, dgs, mtu, flags=FCS, slot=None, slots=None, first=None, base=0, seed=1,
                 aligns=None, l2=None, spare=0, placed=None, front=0, back=0):
        self.mtu, self.flags = mtu, flags
        if placed is None:
            self.arena, self.off, self.ln = pack(dgs, seed, aligns)
            total = sum(fm.plan(d, mtu, flags)[1] for d in dgs)
        else:
            self.arena = np.ascontiguousarray(placed[0], dtype=np.uint8)
            self.off, self.ln = np.asarray(placed[1], dtype=np.uint64), np.asarray(placed[2], dtype=np.uint32)
            buf = self.arena.tobytes()
            pairs, cnt = np.unique(np.stack([self.off, self.ln.astype(np.uint64)]), axis=1, return_counts=True)
            total = sum(fm.plan(buf[int(o):int(o) + int(d)], mtu, flags)[1] * int(c) for (o, d), c in zip(pairs.T, cnt))
        self.n = len(self.off)
        self.l2 = macs_of(self.n, seed + 1) if l2 is None else l2
        self.slot = fm.min_slot(mtu, flags) if slot is None else slot
        self.slots = total + spare if slots is None else slots
        self.first = first
        self.base = 64 + base                      # canary bytes in front of slot 0; `base` sets out's alignment
        rng = np.random.default_rng(seed + 7)
        self.out0 = rng.integers(0, 256, self.base + self.slots * self.slot + 64, dtype=np.uint8)
        exp = self.out0.copy()
        body, self.flen, self.fcs, self.status, self.plan_first = fm.build(
            oracle, inet_oracle, self.arena, self.off, self.ln, self.l2, mtu, flags, self.out0[self.base:], self.slot,
            self.slots, first, frames_fn)
        exp[self.base:] = body
        self.expect = exp
        self.total = total
        self.front = front
        self.around = np.concatenate([rng.integers(0, 256, front, dtype=np.uint8), self.arena,
                                      rng.integers(0, 256, back, dtype=np.uint8)]) if front or back else self.arena

    def run_dev(self, dev, plan=True, flen=True, status=True, fcs=True, stream=None):
        """(arena after, flen, fcs, status, planned first, planned status) of plan_dev + frame_dev."""
        import torch
        if stream is not None:   # the tensors are made and filled on the stream the library works on
            with torch.cuda.stream(stream):
                t = self.launch_dev(dev, plan, flen, status, fcs, stream)
            stream.synchronize()
        else:
            t = self.launch_dev(dev, plan, flen, status, fcs, None)
            torch.cuda.synchronize()
        return self.collect(t)

    def launch_dev(self, dev, plan=True, flen=True, status=True, fcs=True, stream=None):
        """plan_dev + frame_dev, not waited for: the device tensors, for collect() after a synchronise."""
        import torch
        d_arena, d_off, d_ln, d_l2 = (to_dev(x, dev) for x in (self.around, self.off, self.ln, self.l2))
        dg = d_arena.data_ptr() + self.front
        d_out = to_dev(self.out0, dev)
        d_first = torch.full((self.n + 1,), 0x5555555555555555, dtype=torch.int64, device=dev)
        d_pst = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        if plan:
            na.tx_frame_plan_dev(dg, self.arena.size, d_off, d_ln, self.n, self.mtu, d_first, self.flags, d_pst,
                                 stream=stream)
        use_first = d_first if self.first is None else to_dev(np.asarray(self.first, dtype=np.uint64), dev)
        d_flen = torch.full((max(self.slots, 1),), UNSET - (1 << 32), dtype=torch.int32, device=dev)
        d_fcs = torch.full((max(self.slots, 1),), UNSET - (1 << 32), dtype=torch.int32, device=dev)
        d_st = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        na.tx_frame_dev(dg, self.arena.size, d_off, d_ln, d_l2, self.n, self.mtu, use_first,
                        d_out.data_ptr() + self.base, self.slot, self.slots, self.flags, d_flen if flen else None,
                        d_st if status else None, d_fcs if fcs else None, stream=stream)
        return d_out, d_flen, d_fcs, d_st, d_first, d_pst, (d_arena, d_off, d_ln, d_l2, use_first)

    def collect(self, t):
        d_out, d_flen, d_fcs, d_st, d_first, d_pst = t[:6]
        u32 = lambda x, k: x.cpu().numpy().view(np.uint32)[:k]
        return (d_out.cpu().numpy(), u32(d_flen, self.slots), u32(d_fcs, self.slots), u32(d_st, self.n),
                d_first.cpu().numpy().view(np.uint64), u32(d_pst, self.n))

    def run_host(self):
        out = self.out0.copy()
        flen = np.full(max(self.slots, 1), UNSET, dtype=np.uint32)
        st = np.full(max(self.n, 1), 0xFFFFFFFF, dtype=np.uint32)
        k = na.tx_frame_host(self.arena, self.arena.size, self.off, self.ln, self.l2, self.n, self.mtu,
                             out[self.base:], self.slot, self.slots, self.flags, flen, st)
        return out, flen[:self.slots], st[:self.n], k

    def check_dev(self, res):
        out, flen, fcs, st, first, pst = res
        diff = np.flatnonzero(out != self.expect)
        assert diff.size == 0, ("device form", diff[:8], [(int(d) - self.base) // self.slot for d in diff[:8]])
        assert (flen == self.flen).all() and (fcs == self.fcs).all()
        assert (st == self.status).all(), (st[:8], self.status[:8])
        assert (first == self.plan_first).all()
        assert (pst == self.status & ~np.uint32(fm.NO_ROOM)).all()

    def check_host(self):
        hout, hflen, hst, k = self.run_host()
        assert k == self.total
        diff = np.flatnonzero(hout != self.expect)
        assert diff.size == 0, ("host form", diff[:8], [(int(d) - self.base) // self.slot for d in diff[:8]])
        assert (hflen == self.flen).all() and (hst == self.status).all()

    def check(self, dev, host=True):
        self.check_dev(self.run_dev(dev))
        if host and self.first is None and self.total <= self.slots:
            self.check_host()
