"""Batches for the GPU tests of one-pass TCP segmentation (include/nstack_tso.h): a txd_batch.DBatch whose
expected arena, flen, fcs, status and first come from tests/tso_model.py and whose device and host runs
go through ip_tx_tso_plan_dev / ip_tx_tso_dev / ip_tx_tso_host. Also a builder of TCP datagrams and the
"expanded way": ip_tx_frame_l4_dev over the model-expanded datagrams placed at the same slots. Test
infrastructure only."""
import functools
import struct

import numpy as np

import nstack_amd as na
import tso_model as tm
import txf_model as fm
from txd_batch import DBatch
from txf_batch import FCS, UNSET, macs_of, pack, to_dev

_ORACLES = {}


@functools.lru_cache(maxsize=None)
def _frames(dg, mac, mtu, flags, mss):
    return tm.frames(_ORACLES["fcs"], _ORACLES["inet"], dg, mac, mtu, flags, mss)


def frames_fn(fcs_oracle, inet_oracle, dg, mac, mtu, flags, mss):
    """tm.frames, memoised: the frames of a datagram do not depend on where they are placed."""
    _ORACLES["fcs"], _ORACLES["inet"] = fcs_oracle, inet_oracle
    return _frames(bytes(dg), bytes(mac), mtu, flags & ~tm.F_MSS_ONE, mss)


def tcp_datagram(rng, hlen, thl, P, tfl=tm.ACK, foff=0, id0=None, seq0=None, proto=6):
    """A TCP datagram with P payload bytes: IP and TCP options, addresses, ports, both checksum fields and
    the payload are garbage."""
    D = hlen + thl + P
    b = bytearray(rng.integers(0, 256, D, dtype=np.uint8).tobytes())
    b[0] = 0x40 | hlen // 4
    b[2:4] = D.to_bytes(2, "big")
    if id0 is not None:
        b[4:6] = int(id0).to_bytes(2, "big")
    b[6:8] = int(foff).to_bytes(2, "big")
    b[9] = proto
    if seq0 is not None:
        b[hlen + 4:hlen + 8] = int(seq0).to_bytes(4, "big")
    b[hlen + 12] = (thl // 4) << 4 | (b[hlen + 12] & 0x0F)
    b[hlen + 13] = tfl
    return bytes(b)


class TBatch(DBatch):
    """mss: None (the NULL array), an int (TSO_F_MSS_ONE, mss[0] for the batch) or one value per datagram."""

    def __init__(self, oracle, inet_oracle, dgs, mtu, flags=FCS, mss=None, slots=None, spare=0, seed=1, aligns=None,
                 placed=None, **kw):
        if placed is None:
            placed = pack(dgs, seed, aligns)
        arena, off, ln = placed
        buf = np.ascontiguousarray(arena, dtype=np.uint8).tobytes()
        self.dgs = [buf[int(o):int(o) + int(d)] for o, d in zip(off, ln)]
        if mss is None:
            self.mss = None
        elif np.isscalar(mss):
            flags |= tm.F_MSS_ONE
            self.mss = np.array([mss], dtype=np.uint16)
        else:
            self.mss = np.asarray(mss, dtype=np.uint16)
            assert self.mss.size == len(self.dgs)
        l2 = kw.pop("l2", None)
        l2 = macs_of(len(self.dgs), seed + 1) if l2 is None else l2
        macs = np.ascontiguousarray(l2).view(np.uint8).reshape(-1, 12)
        plan = [frames_fn(oracle, inet_oracle, dg, macs[0 if flags & fm.F_L2_ONE else i].tobytes(), mtu, flags,
                          tm.mss_of(self.mss, flags, i)) for i, dg in enumerate(self.dgs)]
        total = sum(len(p[1]) for p in plan)
        super().__init__(oracle, inet_oracle, None, mtu, flags, slots=total + spare if slots is None else slots, seed=seed,
                         placed=placed, l2=l2, **kw)
        self.seed = seed
        self.plan_status = np.array([p[0] for p in plan], dtype=np.uint32)
        self.txd_expect = self.expect          # what ip_tx_frame_l4_dev makes of the same batch, packed by its own plan
        exp = self.out0.copy()
        body, self.flen, self.fcs, self.status, self.plan_first = tm.build(
            oracle, inet_oracle, self.arena, self.off, self.ln, self.l2, self.mss, mtu, flags, self.out0[self.base:],
            self.slot, self.slots, self.first, frames_fn)
        exp[self.base:] = body
        self.expect = exp
        self.total = total

    def d_mss(self, dev):
        return None if self.mss is None else to_dev(self.mss.view(np.int16), dev)

    def launch_dev(self, dev, plan=True, flen=True, status=True, fcs=True, stream=None, call=None):
        import torch
        if call is not None:   # the older calls over the same datagrams (txd_batch.DBatch)
            flags0, self.flags = self.flags, self.flags & tm.TXD_FLAGS
            try:
                return super().launch_dev(dev, plan, flen, status, fcs, stream, call)
            finally:
                self.flags = flags0
        d_arena, d_off, d_ln, d_l2 = (to_dev(x, dev) for x in (self.around, self.off, self.ln, self.l2))
        d_mss = self.d_mss(dev)
        dg = d_arena.data_ptr() + self.front
        d_out = to_dev(self.out0, dev)
        d_first = torch.full((self.n + 1,), 0x5555555555555555, dtype=torch.int64, device=dev)
        d_pst = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        if plan:
            na.tx_tso_plan_dev(dg, self.arena.size, d_off, d_ln, d_mss, self.n, self.mtu, d_first, self.flags, d_pst,
                               stream=stream)
        use_first = d_first if self.first is None else to_dev(np.asarray(self.first, dtype=np.uint64), dev)
        d_flen = torch.full((max(self.slots, 1),), UNSET - (1 << 32), dtype=torch.int32, device=dev)
        d_fcs = torch.full((max(self.slots, 1),), UNSET - (1 << 32), dtype=torch.int32, device=dev)
        d_st = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        na.tx_tso_dev(dg, self.arena.size, d_off, d_ln, d_l2, d_mss, self.n, self.mtu, use_first,
                      d_out.data_ptr() + self.base, self.slot, self.slots, self.flags, d_flen if flen else None,
                      d_st if status else None, d_fcs if fcs else None, stream=stream)
        return d_out, d_flen, d_fcs, d_st, d_first, d_pst, (d_arena, d_off, d_ln, d_l2, use_first, d_mss)

    def run_host(self):
        out = self.out0.copy()
        flen = np.full(max(self.slots, 1), UNSET, dtype=np.uint32)
        st = np.full(max(self.n, 1), 0xFFFFFFFF, dtype=np.uint32)
        k = na.tx_tso_host(self.arena, self.arena.size, self.off, self.ln, self.l2, self.mss, self.n, self.mtu,
                           out[self.base:], self.slot, self.slots, self.flags, flen, st)
        return out, flen[:self.slots], st[:self.n], k

    def check_dev(self, res):
        out, flen, fcs, st, first, pst = res
        diff = np.flatnonzero(out != self.expect)
        assert diff.size == 0, ("device form", diff[:8], [(int(d) - self.base) // self.slot for d in diff[:8]],
                                [(int(d) - self.base) % self.slot for d in diff[:8]])
        assert (flen == self.flen).all()
        assert (fcs == self.fcs).all(), np.flatnonzero(fcs != self.fcs)[:8]
        assert (st == self.status).all(), [(i, hex(st[i]), hex(self.status[i])) for i in np.flatnonzero(st != self.status)[:8]]
        assert (first == self.plan_first).all()
        assert (pst == self.plan_status).all(), [(i, hex(pst[i]), hex(self.plan_status[i]))
                                                 for i in np.flatnonzero(pst != self.plan_status)[:8]]

    def segmented(self):
        return (self.status & tm.SEGMENTED) != 0

    def expanded_way(self, oracle, inet_oracle, dev):
        """The arena ip_tx_frame_l4_dev leaves for the model-expanded datagrams (checksum fields garbage)
        placed at the same slots: segment s of datagram i is a whole datagram at slot first[i] + s."""
        import torch
        assert not (self.status & fm.NO_ROOM).any()
        macs = np.ascontiguousarray(self.l2).view(np.uint8).reshape(-1, 12)
        pf = self.plan_first if self.first is None else self.first
        dgs, first, l2 = [], [], []
        for i, dg in enumerate(self.dgs):
            ex = tm.expand(dg, self.mtu, tm.mss_of(self.mss, self.flags, i), self.flags) or [dg]
            dgs += ex
            first += [int(pf[i]) + s for s in range(len(ex))]
            l2 += [macs[0 if self.flags & fm.F_L2_ONE else i]] * len(ex)
        e = DBatch(oracle, inet_oracle, dgs, self.mtu, self.flags & tm.TXD_FLAGS & ~fm.F_L2_ONE, slot=self.slot,
                   slots=self.slots, first=first, base=self.base - 64, seed=self.seed, l2=np.array(l2, dtype=np.uint8))
        assert np.array_equal(e.out0, self.out0)
        t = e.launch_dev(dev, plan=False)
        torch.cuda.synchronize()
        return e.collect(t)[0]

    def run_txd_dev(self, dev):
        """ip_tx_frame_l4_dev (after ether_tx_frame_plan_dev) over the same batch: (arena after, status)."""
        import torch
        t = self.launch_dev(dev, call=na.tx_frame_l4_dev)
        torch.cuda.synchronize()
        r = self.collect(t)
        return r[0], r[3]


def field(frame: bytes, hlen: int, what: str):
    """A header field of a built frame, by name."""
    T = 14 + hlen
    return {"ip_len": struct.unpack_from(">H", frame, 16)[0], "ip_id": struct.unpack_from(">H", frame, 18)[0],
            "ip_foff": struct.unpack_from(">H", frame, 20)[0], "seq": struct.unpack_from(">I", frame, T + 4)[0],
            "flags": frame[T + 13]}[what]
