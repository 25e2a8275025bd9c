"""Batches for the GPU tests of reassembly with L4 verdicts (include/nstack_rxd.h): an RBatch
(tests/rxr_batch.py: the frames, the canaried output arena and the plain build's expected bytes and
status words) plus the model's verdict words (tests/rxd_model.py). Test infrastructure only."""
import numpy as np

import nstack_amd as na
import rxd_model as rd
from rxr_batch import UNSET, RBatch, mg, to_dev


KINDS = ("udp", "tcp", "icmp")
HLENS = (20, 24, 60)


def whole_mix(inet_oracle, seed=12):
    """Unfragmented frames (with the FCS) of mixed protocols, good and bad: valid datagrams of the three
    kinds, every fourth with a bent last byte, the short segments of every rule, protocol 47, and UDP
    without a checksum."""
    rng = mg.random.Random(seed)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    frames = []
    for q, kind in enumerate(KINDS * 4):
        src, dst = 0x0A000001 + q, 0x0A000101 + q
        seg = rd.segment(inet_oracle, kind, rb(1 + 13 * q), src, dst)
        if q % 4 == 3:
            seg = seg[:-1] + bytes([seg[-1] ^ 0x80])
        frames.append(mg.frame(mg.ip_packet(seg, HLENS[q % 3], ident=q, src=src, dst=dst, proto=rd.PROTO[kind], rng=rng), True))
    for proto, n in ((6, 19), (6, 20), (17, 7), (17, 8), (1, 3), (1, 4), (47, 30), (17, 0), (6, 0), (47, 0)):
        frames.append(mg.frame(mg.ip_packet(rb(n), ident=0x100 + n + proto, proto=proto), True, pad=0))
    udp0 = bytearray(rd.segment(inet_oracle, "udp", rb(20), 1, 2))
    udp0[6:8] = b"\x00\x00"
    frames.append(mg.frame(mg.ip_packet(bytes(udp0), ident=0x200, src=1, dst=2), True))
    return frames


def framed(dev, dgs, mtu, macs):
    """ether_tx_frame_dev over the datagrams, as tests/test_gpu_rxr.py frames them: (device arena of
    slots, slot, first[], flen[]) with the FCS."""
    import torch
    import txf_model as fm
    arena = np.frombuffer(b"".join(dgs), dtype=np.uint8)
    ln = np.array([len(d) for d in dgs], dtype=np.uint32)
    n, slot = len(dgs), fm.min_slot(mtu, fm.F_FCS)
    off = np.zeros(n, dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    d_arena, d_off, d_ln, d_l2 = (to_dev(x, dev) for x in (arena, off, ln, macs))
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    na.tx_frame_plan_dev(d_arena, arena.size, d_off, d_ln, n, mtu, d_first, fm.F_FCS)
    torch.cuda.synchronize()
    first = d_first.cpu().numpy().view(np.uint64)
    slots = int(first[n])
    d_out = torch.full((slots * slot + 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    na.tx_frame_dev(d_arena, arena.size, d_off, d_ln, d_l2, n, mtu, d_first, d_out, slot, slots, fm.F_FCS, d_flen)
    torch.cuda.synchronize()
    return d_out, slot, first, d_flen.cpu().numpy().view(np.uint32)


VARIANTS = ("front", "line", "tail", "src", "dst", "ttl", "hcsum", "behind")


class Traffic:
    """Valid datagrams of the three kinds in three or four fragments each (head header lengths 20, 24
    and 60, the others 20; odd datagram lengths) and three unfragmented ones, all frames with the FCS.
    frames: in datagram order; groups[k]: datagram k's frame indices in offset order; kind[k]."""

    def __init__(self, inet_oracle, seed=21):
        rng = mg.random.Random(seed)
        rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
        self.frames, self.groups, self.kind = [], [], []
        q = 0
        for kind in KINDS:
            for hh in HLENS:
                for cuts, tail in (([24, 64], 5), ([40, 80, 120], 19)):
                    src, dst = 0x0A000001 + 7 * q, 0xC0A80001 + 5 * q
                    hdr = 20 if kind == "tcp" else 8
                    seg = rd.segment(inet_oracle, kind, rb(cuts[-1] + tail + 2 * q - hdr), src, dst)
                    assert (hh + len(seg)) & 1
                    fr = mg.fragments(rng, seg, cuts, True, hlen_head=hh, hlen_rest=20, ident=q, src=src, dst=dst,
                                      proto=rd.PROTO[kind])
                    self._add(fr, kind)
                    q += 1
        for kind, hh in zip(KINDS, HLENS):
            src, dst = 0x0A000001 + 7 * q, 0xC0A80001 + 5 * q
            seg = rd.segment(inet_oracle, kind, rb(41 + 2 * q), src, dst)
            self._add([mg.frame(mg.ip_packet(seg, hh, ident=q, src=src, dst=dst, proto=rd.PROTO[kind], rng=rng), True)], kind)
            q += 1

    def _add(self, fr, kind):
        self.groups.append(list(range(len(self.frames), len(self.frames) + len(fr))))
        self.frames += fr
        self.kind.append(kind)

    # ---- one-bit variants: (frames, the datagrams whose L4 verdict must turn bad) ----
    def bent(self, which, sel):
        """The frames with variant `which` applied to the datagrams of `sel`."""
        frames, hit = list(self.frames), []
        for k in sel:
            g = self.groups[k]
            f0 = self.frames[g[0]]
            hlen0 = (f0[14] & 15) * 4
            flips, turns_bad = [], True
            if which == "front":        # a non-head fragment's first byte: in front of its first 16-byte line unless that begins there
                flips = [(g[1], 34)] if len(g) > 1 else []
            elif which == "line":       # 16 bytes into a non-head fragment of 40 payload bytes: inside a whole line
                flips = [(g[1], 34 + 16)] if len(g) > 1 else [(g[0], 14 + hlen0 + 9)]
            elif which == "tail":       # the datagram's last byte: behind the last fragment's last whole line unless that ends there
                last = self.frames[g[-1]]
                flips = [(g[-1], 14 + int.from_bytes(last[16:18], "big") - 1)] if len(g) > 1 else []
            elif which in ("src", "dst"):   # the address word, in every fragment (the group key); ICMP has no pseudo header
                flips = [(i, 14 + (13 if which == "src" else 18)) for i in g]
                turns_bad = self.kind[k] != "icmp"
            elif which in ("ttl", "hcsum"):  # the header is no part of the L4 sum
                flips, turns_bad = [(g[0], 14 + (8 if which == "ttl" else 10))], False
            elif which == "behind":     # the first padding byte behind ip_len, or else the trailer's last byte
                last = self.frames[g[-1]]
                at = 14 + int.from_bytes(last[16:18], "big")
                flips, turns_bad = [(g[-1], at if at < len(last) - 4 else len(last) - 1)], False
            for i, pos in flips:
                f = bytearray(frames[i])
                f[pos] ^= 0x10
                frames[i] = bytes(f)
            if flips and turns_bad:
                hit.append(k)
        return frames, hit


class DBatch(RBatch):
    def __init__(self, inet_oracle, *a, bad_mask=rd.L4_BAD_CSUM, **kw):
        super().__init__(inet_oracle, *a, **kw)
        self.bad_mask = bad_mask
        self.dverdict = rd.verdicts(inet_oracle, self.expect[self.base:], self.plan, self.out_bytes)
        self.bad = rd.count_bad(self.dverdict, bad_mask)

    # ---- the device form: plan_dev, then the build with sums and the verdict launch ----
    def run_l4_dev(self, dev, bad=True, stream=None):
        import torch
        n1 = max(self.n, 1)
        d_arena = to_dev(self.around if self.around.size else np.zeros(1, np.uint8), dev)
        d_off = to_dev(self.off if self.n else np.zeros(1, np.uint64), dev)
        d_ln = to_dev(self.ln if self.n else np.zeros(1, np.uint32), dev)
        d_v = None if self.verdict is None else to_dev(self.verdict, dev)
        fa = d_arena.data_ptr() + self.front
        t = dict(fstat=torch.full((n1,), -1, dtype=torch.int32, device=dev),
                 dst=torch.full((n1,), 0x5555555555555555, dtype=torch.int64, device=dev),
                 dgi=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 doff=torch.full((self.n + 1,), 0x5555555555555555, dtype=torch.int64, device=dev),
                 dlen=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 dlead=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 counts=torch.full((2,), 0x5555555555555555, dtype=torch.int64, device=dev),
                 final=torch.full((n1,), -1, dtype=torch.int32, device=dev), out=to_dev(self.out0, dev),
                 dverdict=torch.full((n1,), 0x55555555, dtype=torch.int32, device=dev),
                 bad=torch.full((1,), 0x5555555555555555, dtype=torch.int64, device=dev))
        na.rx_reasm_plan_dev(fa, self.arena.size, d_off, d_ln, self.n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"],
                             t["dlead"], t["counts"], flags=self.flags, verdict=d_v, drop_mask=self.drop_mask, align=self.align,
                             stream=stream)
        na.rx_reasm_l4_dev(fa, self.arena.size, d_off, d_ln, self.n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"],
                           t["counts"], t["out"].data_ptr() + self.base, self.out_bytes, t["dverdict"], flags=self.flags,
                           fstat=t["final"], bad_mask=self.bad_mask, bad=t["bad"] if bad else None, stream=stream)
        torch.cuda.synchronize()
        r = self.collect(t)
        r["dverdict"] = t["dverdict"].cpu().numpy().view(np.uint32)
        r["bad"] = int(t["bad"].cpu().numpy().view(np.uint64)[0])
        return r

    def check_l4_dev(self, r, bad=True):
        """The plain build's bytes (canaries included) and final status words, then the verdicts and bad."""
        self.check_dev(r)
        got = r["dverdict"][:self.m]
        assert np.array_equal(got, self.dverdict), ("dverdict", np.flatnonzero(got != self.dverdict)[:8],
                                                    [hex(x) for x in got[:8]], [hex(x) for x in self.dverdict[:8]])
        assert r["bad"] == (self.bad if bad else 0x5555555555555555)

    # ---- the host form ----
    def check_l4_host(self, cut=None):
        """cut: the chunks (datagrams each) the engine must have cut the batch into, asserted first."""
        out = self.out0.copy()
        n1 = max(self.n, 1)
        o = dict(fstat=np.full(n1, 0xFFFFFFFF, np.uint32), doff=np.full(self.n + 1, UNSET, np.uint64),
                 dlen=np.full(n1, UNSET, np.uint32), dlead=np.full(n1, UNSET, np.uint32))
        dv = np.full(n1, UNSET, np.uint32)
        m, bad = na.rx_reasm_l4_host(self.arena, self.arena.size, self.off, self.ln, self.n, out[self.base:], self.out_bytes, dv,
                                     flags=self.flags, verdict=self.verdict, drop_mask=self.drop_mask, align=self.align,
                                     bad_mask=self.bad_mask, **o)
        assert cut is None or na.rxr_last_host_chunks() == cut
        assert m == self.m
        diff = np.flatnonzero(out != self.expect)
        assert diff.size == 0, ("host form", diff[:8] - self.base)
        assert np.array_equal(o["fstat"][:self.n], self.fstat)
        assert np.array_equal(o["doff"][:m + 1], self.plan["doff"]) and np.array_equal(o["dlen"][:m], self.plan["dlen"])
        assert np.array_equal(o["dlead"][:m], self.plan["dlead"])
        assert np.array_equal(dv[:m], self.dverdict), ("host dverdict", np.flatnonzero(dv[:m] != self.dverdict)[:8])
        assert (dv[m:] == UNSET).all() and bad == self.bad
        return dv[:m]
