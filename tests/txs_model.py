"""Expected-result model of one-pass TX sealing: the rule list of include/nstack_txs.h, restated
in Python. It parses with `struct`, takes every CRC and checksum from the oracle
(oracle_ether_fcs, oracle_ip_checksum, oracle_tcp_checksum, oracle_udp_checksum) and has no
arithmetic of its own. Test infrastructure only."""
import socket
import struct

import numpy as np

F_FCS, F_UDP_ZERO = 1, 2
FCS_SET, RUNT, IPV4, IP_BAD_HDR, IP_BAD_LEN, IP_CSUM_SET = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
FRAG, L4_CSUM_SET, L4_SHORT = 0x040, 0x080, 0x200
PROTO_SHIFT = 16
L4_FIELD = {6: 16, 17: 6, 1: 2}   # the checksum field's offset in the segment
FIELDS_DTYPE = np.dtype([("ip_csum", "<u2"), ("l4_csum", "<u2"), ("fcs", "<u4")])


def seal(fcs_oracle, inet_oracle, frame: bytes, flags: int = F_FCS):
    """(bytes after sealing: the F frame bytes and, with F_FCS, the 4 FCS bytes; status word;
    (ip_csum, l4_csum, fcs) as struct txs_fields holds them) of one frame."""
    b = bytearray(frame)
    F = len(b)
    st, ip, l4, fcs = _l3l4(inet_oracle, b, F, flags)
    if flags & F_FCS:                                                    # rule 7
        fcs = fcs_oracle.oracle_ether_fcs(bytes(b), F)
        b += struct.pack("<I", fcs)
        st |= FCS_SET
    return bytes(b), st, (ip, l4, fcs)


def _l3l4(inet_oracle, b: bytearray, F: int, flags: int):
    if F < 14:                                                           # rule 1
        return RUNT, 0, 0, 0
    P = F - 14
    if b[12] != 0x08 or b[13] != 0x00:                                   # rule 2
        return 0, 0, 0, 0
    st = IPV4
    if P < 20:                                                           # rule 3
        return st | IP_BAD_HDR, 0, 0, 0
    vhl, _tos, ip_len, _id, foff, _ttl, proto, _csum = struct.unpack_from(">BBHHHBBH", b, 14)
    hlen = (vhl & 0x0F) * 4
    if (vhl & 0x40) != 0x40 or hlen < 20 or hlen > P:
        return st | IP_BAD_HDR, 0, 0, 0
    st |= (proto << PROTO_SHIFT) | IP_CSUM_SET
    b[24:26] = b"\x00\x00"
    ip = inet_oracle.oracle_ip_checksum(bytes(b[14:14 + hlen]), hlen)
    b[24:26] = struct.pack("<H", ip)                                     # the uint16_t as it is (ip.c:79-80)
    bad_len = ip_len < hlen or ip_len > P                                # rule 4
    if bad_len:
        st |= IP_BAD_LEN
    if foff & 0x3FFF:                                                    # rule 5
        st |= FRAG
    if bad_len or foff & 0x3FFF:
        return st, ip, 0, 0
    L = ip_len - hlen                                                    # rule 6
    s0 = 14 + hlen
    if proto not in L4_FIELD:
        return st, ip, 0, 0
    if L < {6: 20, 17: 8, 1: 4}[proto]:
        return st | L4_SHORT, ip, 0, 0
    q = s0 + L4_FIELD[proto]
    b[q:q + 2] = b"\x00\x00"
    src_raw, dst_raw = struct.unpack_from("<II", b, 26)                  # in_addr_t words as they lie
    seg = bytes(b[s0:s0 + L])
    if proto == 6:
        l4 = inet_oracle.oracle_tcp_checksum(socket.ntohl(src_raw), socket.ntohl(dst_raw), seg, L)
    elif proto == 17:
        if flags & F_UDP_ZERO:
            return st, ip, 0, 0                                          # the zero stays: "no checksum"
        l4 = inet_oracle.oracle_udp_checksum(seg, L, src_raw, dst_raw) or 0xFFFF   # RFC 768
    else:
        l4 = inet_oracle.oracle_ip_checksum(seg, L)
    b[q:q + 2] = struct.pack("<H", l4)
    return st | L4_CSUM_SET, ip, l4, 0


def seal_arena(fcs_oracle, inet_oracle, arena, off, ln, flags: int = F_FCS):
    """(sealed copy of the arena, status words, fields records) of a batch."""
    out = np.array(arena, dtype=np.uint8, copy=True)
    buf = out.tobytes()
    n = len(off)
    status = np.zeros(n, dtype=np.uint32)
    fields = np.zeros(n, dtype=FIELDS_DTYPE)
    for i, (o, l) in enumerate(zip(off, ln)):
        o, l = int(o), int(l)
        sealed, st, fl = seal(fcs_oracle, inet_oracle, buf[o:o + l], flags)
        out[o:o + len(sealed)] = np.frombuffer(sealed, dtype=np.uint8)
        status[i] = st
        fields[i] = fl
    return out, status, fields
