"""Expected-result model of one-pass TCP segmentation: the rule list of include/nstack_tso.h, restated in
Python. `expand` cuts a segmented datagram into its per-segment datagrams by plain byte surgery and
leaves both checksum fields as garbage; tests/txd_model.py (the oracle's checksum functions) and
tests/txf_model.py then frame each of them whole. Everything that is not segmented is txd_model.frames
of the datagram itself. No checksum arithmetic of its own. Test infrastructure only."""
import struct

import numpy as np

import txd_model as dm
import txf_model as fm

F_ID_FIXED, F_MSS_ONE = 0x200, 0x400
SEGMENTED = 0x400
MAX_HDR = 114
FIN, SYN, RST, PSH, ACK, URG, ECE, CWR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
TXD_FLAGS = dm.TXF_FLAGS | dm.F_UDP_ZERO
GARBAGE = b"\xde\xad"   # what expand leaves in both checksum fields: the filling ignores it


def unit(dg: bytes, mtu: int, mss: int = 0):
    """(m, thl) of a datagram rule 3 segments, None for every other one (rules 1-3)."""
    st, _cnt, hlen, _mx = fm.plan(dg, mtu, 0)
    if st & (fm.BAD_HDR | fm.BAD_LEN):
        return None
    foff = struct.unpack_from(">H", dg, 6)[0]
    L = len(dg) - hlen
    if dg[9] != 6 or foff & 0x3FFF or L < 20:
        return None
    thl = (dg[hlen + 12] >> 4) * 4
    if thl < 20 or thl > L or hlen + thl > MAX_HDR or dg[hlen + 13] & (SYN | RST | URG):
        return None
    cap = mtu - hlen - thl
    if cap < 1:
        return None
    m = min(mss or cap, cap)
    return (m, thl) if L - thl > m else None


def count(dg: bytes, mtu: int, mss: int = 0) -> int:
    u = unit(dg, mtu, mss)
    if u is None:
        return 0
    return -(-(len(dg) - (dg[0] & 15) * 4 - u[1]) // u[0])


def expand(dg: bytes, mtu: int, mss: int = 0, flags: int = 0):
    """The per-segment datagrams of rule 4, or None for a datagram that is not segmented."""
    u = unit(dg, mtu, mss)
    if u is None:
        return None
    m, thl = u
    hlen = (dg[0] & 15) * 4
    hb = hlen + thl
    P = len(dg) - hb
    id0 = struct.unpack_from(">H", dg, 4)[0]
    seq0 = struct.unpack_from(">I", dg, hlen + 4)[0]
    cnt = -(-P // m)
    out = []
    for s in range(cnt):
        pay = dg[hb + s * m:hb + (s + 1) * m]
        h = bytearray(dg[:hb])
        struct.pack_into(">H", h, 2, hb + len(pay))
        struct.pack_into(">H", h, 4, id0 if flags & F_ID_FIXED else (id0 + s) & 0xFFFF)
        h[10:12] = GARBAGE
        struct.pack_into(">I", h, hlen + 4, (seq0 + s * m) & 0xFFFFFFFF)
        if s < cnt - 1:
            h[hlen + 13] &= ~(FIN | PSH) & 0xFF
        if s > 0:
            h[hlen + 13] &= ~CWR & 0xFF
        h[hlen + 16:hlen + 18] = GARBAGE
        out.append(bytes(h) + pay)
    return out


def frames(fcs_oracle, inet_oracle, dg: bytes, mac: bytes, mtu: int, flags: int = fm.F_FCS, mss: int = 0):
    """(status, frames, fcs values) as txd_model.frames gives them."""
    ex = expand(dg, mtu, mss, flags)
    if ex is None:
        return dm.frames(fcs_oracle, inet_oracle, dg, mac, mtu, flags & TXD_FLAGS)
    out, crcs = [], []
    for e in ex:
        st, fr, cr = dm.frames(fcs_oracle, inet_oracle, e, mac, mtu, flags & dm.TXF_FLAGS)
        assert st == fm.WHOLE | dm.L4_CSUM_SET | 6 << dm.PROTO_SHIFT and len(fr) == 1
        out += fr
        crcs += cr
    return SEGMENTED | dm.L4_CSUM_SET | 6 << dm.PROTO_SHIFT, out, crcs                # rule 6


def mss_of(mss, flags, i):
    if mss is None:
        return 0
    return int(mss[0 if flags & F_MSS_ONE else i])


def build(fcs_oracle, inet_oracle, dgram, off, ln, l2, mss, mtu, flags, out, slot, slots, first=None, frames_fn=None):
    """txd_model.build with this module's frames: (arena after the call, flen, fcs, status, first). The
    datagram's mss travels to frames_fn through a per-datagram closure, since txf_model.build's frames_fn
    takes no index."""
    frames_fn = frames_fn or frames
    it = iter(range(len(off)))

    def fn(fo, io, dg, mac, mtu_, flags_):
        return frames_fn(fo, io, dg, mac, mtu_, flags_, mss_of(mss, flags, next(it)))

    res = list(fm.build(fcs_oracle, inet_oracle, dgram, off, ln, l2, mtu, flags, out, slot, slots, first, fn))
    status = res[3]
    for i in range(len(status)):
        if int(status[i]) & fm.NO_ROOM:
            status[i] = int(status[i]) & ~(dm.L4_CSUM_SET | dm.L4_SHORT)
    return tuple(res)


def plan_status(inet_oracle, dgs, mtu, flags, mss=None):
    """The status words and first[] the plan call writes (rule 6: the whole word, without TXF_NO_ROOM)."""
    st, first, k = [], [], 0
    for i, dg in enumerate(dgs):
        s, fr, _ = frames(None, inet_oracle, dg, bytes(12), mtu, flags & ~fm.F_FCS, mss_of(mss, flags, i))
        st.append(s)
        first.append(k)
        k += len(fr)
    return np.array(st, dtype=np.uint32), np.array(first + [k], dtype=np.uint64)
