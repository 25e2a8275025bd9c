"""Batches for the GPU tests of TX framing with L4 checksums (include/nstack_txd.h): a txf_batch.Batch
whose expected arena, flen, fcs and status come from tests/txd_model.py and whose device and host
runs go through ip_tx_frame_l4_dev / ip_tx_frame_l4_host. Also builders of datagrams with an L4
protocol. Test infrastructure only."""
import functools
import struct

import numpy as np

import nstack_amd as na
import txd_model as dm
import txf_model as fm
from txf_batch import FCS, UNSET, Batch, to_dev

PROTO = {"tcp": 6, "udp": 17, "icmp": 1}
_ORACLES = {}


@functools.lru_cache(maxsize=None)
def _frames(dg, mac, mtu, flags):
    return dm.frames(_ORACLES["fcs"], _ORACLES["inet"], dg, mac, mtu, flags)


def frames_fn(fcs_oracle, inet_oracle, dg, mac, mtu, flags):
    """dm.frames, memoised: the frames of a datagram do not depend on where they are placed."""
    _ORACLES["fcs"], _ORACLES["inet"] = fcs_oracle, inet_oracle
    return _frames(bytes(dg), bytes(mac), mtu, flags)


def l4_datagram(rng, proto, hlen, L, foff=0, seg=None):
    """An IPv4 datagram of `proto` with an L-byte segment of random bytes (or `seg`): options, addresses,
    both checksum fields and the payload are garbage."""
    D = hlen + L
    b = bytearray(rng.integers(0, 256, D, dtype=np.uint8).tobytes())
    b[0] = 0x40 | hlen // 4
    b[2:4] = D.to_bytes(2, "big")
    b[6:8] = int(foff).to_bytes(2, "big")
    b[9] = proto
    if seg is not None:
        b[hlen:] = seg
    return bytes(b)


def udp_summing_to_zero(inet_oracle, rng, hlen, n):
    """A UDP datagram with n payload bytes (n >= 2) whose computed checksum is 0, so 0xffff is stored:
    two payload bytes are set to what udp_checksum returns for the rest."""
    dg = bytearray(l4_datagram(rng, 17, hlen, 8 + n))
    dg[hlen + 6:hlen + 10] = b"\x00\x00\x00\x00"
    src_raw, dst_raw = struct.unpack_from("<II", dg, 12)
    c = inet_oracle.oracle_udp_checksum(bytes(dg[hlen:]), 8 + n, src_raw, dst_raw)
    dg[hlen + 8:hlen + 10] = struct.pack("<H", c)
    assert inet_oracle.oracle_udp_checksum(bytes(dg[hlen:]), 8 + n, src_raw, dst_raw) == 0
    dg[hlen + 6:hlen + 8] = b"\x5a\xa5"       # field garbage: ignored
    return bytes(dg)


class DBatch(Batch):
    def __init__(self, oracle, inet_oracle, dgs, mtu, flags=FCS, **kw):
        super().__init__(oracle, inet_oracle, dgs, mtu, flags, **kw)
        # what ether_tx_frame_dev makes of the same batch (the datagrams as they are)
        self.txf_expect, self.txf_status = self.expect, self.status
        exp = self.out0.copy()
        body, self.flen, self.fcs, self.status, self.plan_first = dm.build(
            oracle, inet_oracle, self.arena, self.off, self.ln, self.l2, mtu, flags, self.out0[self.base:], self.slot,
            self.slots, self.first, frames_fn)
        exp[self.base:] = body
        self.expect = exp

    def launch_dev(self, dev, plan=True, flen=True, status=True, fcs=True, stream=None, call=None):
        import torch
        call = call or na.tx_frame_l4_dev
        flags = self.flags if call is na.tx_frame_l4_dev else self.flags & dm.TXF_FLAGS
        d_arena, d_off, d_ln, d_l2 = (to_dev(x, dev) for x in (self.around, self.off, self.ln, self.l2))
        dg = d_arena.data_ptr() + self.front
        d_out = to_dev(self.out0, dev)
        d_first = torch.full((self.n + 1,), 0x5555555555555555, dtype=torch.int64, device=dev)
        d_pst = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        if plan:
            na.tx_frame_plan_dev(dg, self.arena.size, d_off, d_ln, self.n, self.mtu, d_first, self.flags & dm.TXF_FLAGS,
                                 d_pst, stream=stream)
        use_first = d_first if self.first is None else to_dev(np.asarray(self.first, dtype=np.uint64), dev)
        d_flen = torch.full((max(self.slots, 1),), UNSET - (1 << 32), dtype=torch.int32, device=dev)
        d_fcs = torch.full((max(self.slots, 1),), UNSET - (1 << 32), dtype=torch.int32, device=dev)
        d_st = torch.full((max(self.n, 1),), -1, dtype=torch.int32, device=dev)
        call(dg, self.arena.size, d_off, d_ln, d_l2, self.n, self.mtu, use_first, d_out.data_ptr() + self.base, self.slot,
             self.slots, flags, d_flen if flen else None, d_st if status else None, d_fcs if fcs else None, stream=stream)
        return d_out, d_flen, d_fcs, d_st, d_first, d_pst, (d_arena, d_off, d_ln, d_l2, use_first)

    def run_txf_dev(self, dev):
        """ether_tx_frame_dev over the same batch: (arena after, status)."""
        import torch
        t = self.launch_dev(dev, call=na.tx_frame_dev)
        torch.cuda.synchronize()
        r = self.collect(t)
        return r[0], r[3]

    def run_host(self):
        out = self.out0.copy()
        flen = np.full(max(self.slots, 1), UNSET, dtype=np.uint32)
        st = np.full(max(self.n, 1), 0xFFFFFFFF, dtype=np.uint32)
        k = na.tx_frame_l4_host(self.arena, self.arena.size, self.off, self.ln, self.l2, self.n, self.mtu,
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
        assert (pst == self.txf_status & ~np.uint32(fm.NO_ROOM)).all()
