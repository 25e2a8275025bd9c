"""Batches for the tests of one-pass RX coalescing (include/nstack_gro.h): the frames in an arena, the
canaried output arena and the model's result (tests/gro_model.py) for one placement, with the device
and host calls checked against it as tests/rxd_batch.py checks reassembly. Also the traffic the tests
share. Test infrastructure only."""
import numpy as np

import gro_model as gm
import nstack_amd as na
import rxd_model as rd
import rxr_model as rr
from rxd_batch import DBatch
from rxr_batch import UNSET, classify_fn, mg, to_dev


class GBatch(DBatch):
    """RBatch's fields with gro_model's plan, bytes, status words and verdict words."""

    def __init__(self, inet_oracle, frames=None, flags=0, verdict=None, drop_mask=0, align=1, lead=0, gap=0, order=None,
                 out_base=0, out_bytes=None, seed=1, placed=None, bad_mask=rd.L4_BAD_CSUM):
        self.flags, self.drop_mask, self.align, self.bad_mask = flags, drop_mask, align, bad_mask
        if placed is None:
            self.arena, self.off, self.ln = rr.layout(frames, lead=lead, gap=gap, order=order)
            if not frames:
                self.arena = self.arena[:lead]
        else:
            self.arena = np.ascontiguousarray(placed[0], dtype=np.uint8)
            self.off, self.ln = np.asarray(placed[1], dtype=np.uint64), np.asarray(placed[2], dtype=np.uint32)
            buf = self.arena.tobytes()
            frames = [buf[int(o):int(o) + int(d)] for o, d in zip(self.off, self.ln)]
        self.frames, self.n = frames, len(frames)
        self.verdict = None if verdict is None else np.asarray(verdict, dtype=np.uint32)
        self.plan = gm.plan(frames, flags, self.verdict, drop_mask, align, classify_fn)
        self.m = self.plan["m"]
        self.need = int(self.plan["doff"][self.m - 1]) + int(self.plan["dlen"][self.m - 1]) if self.m else 0
        self.out_bytes = self.need if out_bytes is None else out_bytes
        self.base = 64 + out_base                  # canary bytes in front of `out`
        rng = np.random.default_rng(seed + 7)
        self.out0 = rng.integers(0, 256, self.base + max(self.out_bytes, int(self.plan["doff"][self.m])) + 64, dtype=np.uint8)
        body, self.fstat = gm.build(inet_oracle, frames, self.plan, self.out0[self.base:], self.out_bytes)
        self.expect = self.out0.copy()
        self.expect[self.base:] = body
        self.front, self.around = 0, self.arena
        self.dverdict = gm.verdicts(inet_oracle, self.expect[self.base:], self.plan, self.out_bytes)
        self.bad = rd.count_bad(self.dverdict, bad_mask)

    def datagrams(self, arena=None):
        """The delivered datagrams of an output arena (default: the expected one), in datagram order."""
        body = (self.expect if arena is None else arena)[self.base:]
        return rr.datagrams(body, self.plan)

    # ---- the device form: gro plan, then the coalescing build and the finishing launch ----
    def run_gro_dev(self, dev, bad=True, dlead=True, final=True, plan_only=False, reference=False):
        """reference: the existing plan plus ip_rx_reasm_l4_dev on the same frames instead."""
        import torch
        n1 = max(self.n, 1)
        d_arena = to_dev(self.arena if self.arena.size else np.zeros(1, np.uint8), dev)
        d_off = to_dev(self.off if self.n else np.zeros(1, np.uint64), dev)
        d_ln = to_dev(self.ln if self.n else np.zeros(1, np.uint32), dev)
        d_v = None if self.verdict is None else to_dev(self.verdict, dev)
        fa = d_arena.data_ptr()
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
        plan_fn, build_fn = (na.rx_reasm_plan_dev, na.rx_reasm_l4_dev) if reference else (na.rx_gro_plan_dev, na.rx_gro_dev)
        plan_fn(fa, self.arena.size, d_off, d_ln, self.n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"],
                t["dlead"] if dlead else None, t["counts"], flags=self.flags, verdict=d_v, drop_mask=self.drop_mask, align=self.align)
        if not plan_only:
            build_fn(fa, self.arena.size, d_off, d_ln, self.n, t["fstat"], t["dst"], t["dgi"], t["doff"], t["dlen"], t["counts"],
                     t["out"].data_ptr() + self.base, self.out_bytes, t["dverdict"], flags=self.flags,
                     fstat=t["final"] if final else None, bad_mask=self.bad_mask, bad=t["bad"] if bad else None)
        torch.cuda.synchronize()
        r = self.collect(t)
        r["dverdict"] = t["dverdict"].cpu().numpy().view(np.uint32)
        r["bad"] = int(t["bad"].cpu().numpy().view(np.uint64)[0])
        return r

    def check_gro_dev(self, r, bad=True, dlead=True, final=True):
        """The plan arrays, the whole output arena (canaries included), the final status words, the verdicts and bad."""
        self.check_dev(r, fstat=final, dlead=dlead)
        got = r["dverdict"][:self.m]
        assert np.array_equal(got, self.dverdict), ("dverdict", np.flatnonzero(got != self.dverdict)[:8],
                                                    [hex(x) for x in got[:8]], [hex(x) for x in self.dverdict[:8]])
        assert (r["dverdict"][self.m:self.n] == 0).all()
        assert r["bad"] == (self.bad if bad else 0x5555555555555555)

    # ---- the host plan ----
    def check_plan_host(self):
        n1 = max(self.n, 1)
        o = dict(fstat=np.full(n1, UNSET, np.uint32), dst=np.full(n1, UNSET, np.uint64), dgi=np.full(n1, UNSET, np.uint32),
                 doff=np.full(self.n + 1, UNSET, np.uint64), dlen=np.full(n1, UNSET, np.uint32), dlead=np.full(n1, UNSET, np.uint32))
        m = na.rx_gro_plan_host(self.arena, self.arena.size, self.off, self.ln, self.n, flags=self.flags, verdict=self.verdict,
                                drop_mask=self.drop_mask, align=self.align, **o)
        assert m == self.m
        o["counts"] = np.array([m, int(o["doff"][m])], dtype=np.uint64)
        self.check_plan(o)

    # ---- the host form ----
    def check_gro_host(self, cut=None):
        out = self.out0.copy()
        n1 = max(self.n, 1)
        o = dict(fstat=np.full(n1, 0xFFFFFFFF, np.uint32), doff=np.full(self.n + 1, UNSET, np.uint64),
                 dlen=np.full(n1, UNSET, np.uint32), dlead=np.full(n1, UNSET, np.uint32))
        dv = np.full(n1, UNSET, np.uint32)
        m, bad = na.rx_gro_host(self.arena, self.arena.size, self.off, self.ln, self.n, out[self.base:], self.out_bytes, dv,
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


# ---- traffic ----
def cut(inet_oracle, dg: bytes, mss: int, id_fixed=False, trailer=False, pad=46):
    """The frames nstack_tso.h rule 4 makes of a TCP datagram at this mss, with the checksums the oracle
    computes: tests/tso_model.expand's byte surgery, then both fields filled."""
    import struct

    import tso_model as tm
    ex = tm.expand(dg, 65535, mss, tm.F_ID_FIXED if id_fixed else 0) or [dg]
    out = []
    for e in ex:
        e = bytearray(e)
        hlen = (e[0] & 15) * 4
        e[10:12] = b"\x00\x00"
        e[10:12] = struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(e[:hlen]), hlen))
        e[hlen + 16:hlen + 18] = b"\x00\x00"
        src, dst = struct.unpack_from(">II", e, 12)
        e[hlen + 16:hlen + 18] = struct.pack("<H", inet_oracle.oracle_tcp_checksum(src, dst, bytes(e[hlen:]), len(e) - hlen))
        out.append(mg.frame(bytes(e), trailer, pad=pad))
    return out


def payload(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


ALL_FLAGS = gm.ACK | gm.PSH | gm.FIN | gm.CWR | gm.ECE
SEQ0S = (0, 5 << 15, (1 << 32) - (1 << 15))


def tso_datagrams(inet_oracle, mss, seed=3):
    """Valid TCP datagrams for the round trip with segmentation at `mss`: seq0 a multiple of 32768
    (2^32 - 32768 among them), hlen 20 or 24, thl 20, 32 or 60, every flag segmentation touches, payloads
    around the mss and, for the larger units, up to 32768 minus the headers. Each is a flow of its own."""
    rng = np.random.default_rng(seed + mss)
    shapes = [(20, 20), (24, 32), (20, 60), (24, 60), (20, 32), (24, 20)]
    if mss >= 536:
        ps = [1, mss, mss + 1, 2 * mss + 7, None, 3 * mss]
    else:
        ps = [1, mss + 1, 8 * mss + 3, 29, 40 * mss, 17 * mss + (mss > 1)]
    out = []
    for q, ((hlen, thl), P) in enumerate(zip(shapes, ps)):
        P = 32768 - hlen - thl if P is None else P
        out.append(gm.tcp_datagram(inet_oracle, payload(rng, P), SEQ0S[q % 3], hlen, thl, ALL_FLAGS, sport=0x8000 + q,
                                   ident=0xFFF0 + 3 * q, src=0x0A000001 + q))
    return out


def stays_apart(inet_oracle, seed=11):
    """(frames, verdict, drop_mask, cases): one group each that rule 3 refuses or rule 2 keeps out, every
    case a flow of its own; cases[name] = its frame indices. Every frame must come out alone."""
    rng = np.random.default_rng(seed)
    frames, cases, verdict = [], {}, []
    flow = [0]

    def seg(seq, P, **kw):
        kw.setdefault("sport", 0x9000 + flow[0])
        return mg.frame(gm.tcp_datagram(inet_oracle, payload(rng, P), seq, **kw), False)

    def add(name, frs, drop=()):
        cases[name] = list(range(len(frames), len(frames) + len(frs)))
        verdict.extend(0x21 if q in drop else 0x40 for q in range(len(frs)))
        frames.extend(frs)
        flow[0] += 1

    add("gap", [seg(0, 100), seg(101, 50)])
    add("duplicate", [seg(0, 100), seg(100, 50), seg(100, 50)])
    add("overlap", [seg(0, 100), seg(50, 100)])
    add("balanced", [seg(0, 100), seg(50, 100), seg(200, 50)])
    add("ack", [seg(0, 100), seg(100, 50, ack=0x0A0B0C0E)])
    add("window", [seg(0, 100), seg(100, 50, window=0x2001)])
    add("option", [seg(0, 100, thl=24), seg(100, 50, thl=24, tcpopt=b"\x41\x42\x43\x45")])
    add("ttl", [seg(0, 100), seg(100, 50, ttl=63)])
    add("tos", [seg(0, 100), seg(100, 50, tos=4)])
    add("df", [seg(0, 100), seg(100, 50, foff=0x4000)])
    add("hlen", [seg(0, 100), seg(100, 50, hlen=24)])
    add("thl", [seg(0, 100), seg(100, 50, thl=24)])
    add("fin_mid", [seg(0, 100, tflags=gm.ACK | gm.FIN), seg(100, 50)])
    add("psh_mid", [seg(0, 100, tflags=gm.ACK | gm.PSH), seg(100, 50)])
    add("cwr_later", [seg(0, 100), seg(100, 50, tflags=gm.ACK | gm.CWR)])
    add("syn", [seg(0, 100), seg(100, 50, tflags=gm.ACK | gm.SYN)])
    add("rst", [seg(0, 100), seg(100, 50, tflags=gm.ACK | gm.RST)])
    add("urg", [seg(0, 100, tflags=gm.ACK | gm.URG), seg(100, 50)])
    add("p0", [seg(0, 100), mg.frame(gm.tcp_datagram(inet_oracle, b"", 100, sport=0x9000 + flow[0]), False)])
    add("dropped", [seg(0, 100), seg(100, 50), seg(150, 25)], drop=(1,))
    add("other_addr", [seg(0, 100, sport=0x7777), seg(100, 50, sport=0x7777, src=0x0A0000FE)])
    add("other_port", [seg(0, 100, sport=0x7778), seg(100, 50, sport=0x7779)])
    return frames, np.array(verdict, dtype=np.uint32), 0x3B, cases


def mixed_no_group(inet_oracle, seed=13):
    """Fragments (UDP and TCP), ICMP, non-IPv4 frames, runts and lone segments, with the FCS: nothing coalescible."""
    rng = mg.random.Random(seed)
    nrng = np.random.default_rng(seed)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    udp = rd.segment(inet_oracle, "udp", rb(90), 1, 2)
    tcp = rd.segment(inet_oracle, "tcp", rb(130), 3, 4)
    icmp = rd.segment(inet_oracle, "icmp", rb(40), 5, 6)
    fr = mg.fragments(rng, udp, [48], True, ident=1, src=1, dst=2)[::-1]
    fr += mg.fragments(rng, tcp, [64, 128], True, hlen_head=24, ident=2, src=3, dst=4, proto=6)
    fr.append(mg.frame(mg.ip_packet(icmp, ident=3, src=5, dst=6, proto=1), True))
    fr += [mg.frame(rb(28), True, etype=0x0806), mg.frame(b"\x60" + rb(45), True, etype=0x86DD), rb(13), rb(17)]
    for q, P in enumerate((1, 100, 1460, 0)):                            # lone segments, one flow each; the last a pure ACK
        fr.append(mg.frame(gm.tcp_datagram(inet_oracle, payload(nrng, P), 1000 * q, sport=0xA000 + q, hlen=20 + 4 * (q & 1)), True))
    fr.append(mg.frame(gm.tcp_datagram(inet_oracle, payload(nrng, 9), 7, sport=0xA100)[:-1] + b"\x00", True))   # a bad checksum
    fr += mg.fragments(rng, rb(64), [32], True, ident=9, proto=6)[:1]   # a lone TCP head fragment
    return fr
