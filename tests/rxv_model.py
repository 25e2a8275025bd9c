"""Expected-verdict model of the one-pass RX validator: the rule list of include/nstack_rxv.h,
restated in Python. It parses with `struct`, takes every CRC and checksum from the oracle
(oracle_ether_fcs, oracle_ip_checksum, oracle_tcp_checksum, oracle_udp_checksum) and has no
arithmetic of its own. Test infrastructure only."""
import socket
import struct

import numpy as np

F_TRAILER = 1
FCS_BAD, RUNT, IPV4, IP_BAD_HDR, IP_BAD_LEN, IP_BAD_CSUM = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
FRAG, L4_CHECKED, L4_BAD_CSUM, L4_SHORT = 0x040, 0x080, 0x100, 0x200
PROTO_SHIFT = 16
RESIDUE = 0x2144DF1C


class Parsed:
    """What the model read from a frame whose L4 checksum it evaluated (for the cross-checks)."""

    def __init__(self, proto, l4_off, l4_len, src, dst):
        self.proto, self.l4_off, self.l4_len, self.src, self.dst = proto, l4_off, l4_len, src, dst


def verdict(fcs_oracle, inet_oracle, frame: bytes, flags: int = F_TRAILER, parsed=None) -> int:
    """The verdict word of one frame. `parsed` (a list) receives a Parsed when L4_CHECKED is set."""
    F = len(frame)
    T = 4 if flags & F_TRAILER else 0
    v = 0
    if T and fcs_oracle.oracle_ether_fcs(frame, F) != RESIDUE:          # rule 1
        v |= FCS_BAD
    if F < 14 + T:                                                       # rule 2
        return v | RUNT
    P = F - 14 - T
    (ethertype,) = struct.unpack_from(">H", frame, 12)                   # rule 3
    if ethertype != 0x0800:
        return v
    v |= IPV4
    if P < 20:                                                           # rule 4
        return v | IP_BAD_HDR
    vhl, _tos, ip_len, _id, foff, _ttl, proto, _csum = struct.unpack_from(">BBHHHBBH", frame, 14)
    src_raw, dst_raw = struct.unpack_from("<II", frame, 26)              # in_addr_t words as they lie
    hlen = (vhl & 0x0F) * 4
    if (vhl & 0x40) != 0x40 or hlen < 20 or hlen > P:
        return v | IP_BAD_HDR
    v |= proto << PROTO_SHIFT
    if ip_len != P:                                                      # rule 5
        v |= IP_BAD_LEN
    if inet_oracle.oracle_ip_checksum(frame[14:14 + hlen], hlen) != 0:   # rule 6
        v |= IP_BAD_CSUM
    if foff & 0x2000 or foff & 0x1FFF:                                   # rule 7
        return v | FRAG
    if not hlen <= ip_len <= P:                                          # rule 8
        return v
    L = ip_len - hlen
    seg = frame[14 + hlen:14 + ip_len]
    bad = None
    if proto == 6:
        if L < 20:
            return v | L4_SHORT
        bad = inet_oracle.oracle_tcp_checksum(socket.ntohl(src_raw), socket.ntohl(dst_raw), seg, L) != 0
    elif proto == 17:
        if L < 8:
            return v | L4_SHORT
        if seg[6:8] != b"\x00\x00":
            bad = inet_oracle.oracle_udp_checksum(seg, L, src_raw, dst_raw) != 0
    elif proto == 1:
        if L < 4:
            return v | L4_SHORT
        bad = inet_oracle.oracle_ip_checksum(seg, L) != 0
    if bad is not None:
        v |= L4_CHECKED
        if bad:
            v |= L4_BAD_CSUM
        if parsed is not None:
            parsed.append(Parsed(proto, 14 + hlen, L, src_raw, dst_raw))
    return v


def verdicts(fcs_oracle, inet_oracle, arena, off, ln, flags: int = F_TRAILER) -> np.ndarray:
    """The verdict words of a batch (arena: bytes-like or uint8 array)."""
    buf = arena.tobytes() if isinstance(arena, np.ndarray) else bytes(arena)
    return np.array([verdict(fcs_oracle, inet_oracle, buf[int(o):int(o) + int(l)], flags) for o, l in zip(off, ln)],
                    dtype=np.uint32)
