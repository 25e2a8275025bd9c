"""Expected-result model of TX framing with L4 checksums: the rule list of include/nstack_txd.h,
restated in Python. It fills the L4 field of a datagram with the oracle's own functions
(oracle_tcp_checksum, oracle_udp_checksum, oracle_ip_checksum), then frames the result with
tests/txf_model.py; it has no arithmetic of its own. Test infrastructure only."""
import socket
import struct

import txf_model as fm

F_UDP_ZERO = 0x100
L4_CSUM_SET, L4_SHORT = 0x080, 0x200
PROTO_SHIFT = 16
L4_FIELD = {6: 16, 17: 6, 1: 2}   # the checksum field's offset in the segment
L4_MIN = {6: 20, 17: 8, 1: 4}     # the shortest segment that has the field
TXF_FLAGS = fm.F_FCS | fm.F_HONOR_DF | fm.F_L2_ONE


def fill(inet_oracle, dg: bytes, mtu: int, flags: int = 0):
    """(the datagram with its L4 field as rule 3 leaves it, the bits rule 4 adds to the status word)."""
    st, cnt, hlen, _mx = fm.plan(dg, mtu, flags & TXF_FLAGS)
    if st & (fm.BAD_HDR | fm.BAD_LEN):
        return dg, 0
    proto = dg[9]
    bits = proto << PROTO_SHIFT
    foff = struct.unpack_from(">H", dg, 6)[0]
    if cnt == 0 or foff & 0x3FFF or proto not in L4_FIELD:                # rule 2
        return dg, bits
    L = len(dg) - hlen
    if L < L4_MIN[proto]:
        return dg, bits | L4_SHORT
    b = bytearray(dg)
    q = hlen + L4_FIELD[proto]
    b[q:q + 2] = b"\x00\x00"                                             # the old content is ignored
    src_raw, dst_raw = struct.unpack_from("<II", b, 12)                  # in_addr_t words as they lie
    seg = bytes(b[hlen:])
    if proto == 6:
        l4 = inet_oracle.oracle_tcp_checksum(socket.ntohl(src_raw), socket.ntohl(dst_raw), seg, L)
    elif proto == 17:
        if flags & F_UDP_ZERO:
            return bytes(b), bits                                        # the zero stays: "no checksum"
        l4 = inet_oracle.oracle_udp_checksum(seg, L, src_raw, dst_raw) or 0xFFFF   # RFC 768
    else:
        l4 = inet_oracle.oracle_ip_checksum(seg, L)
    b[q:q + 2] = struct.pack("<H", l4)
    return bytes(b), bits | L4_CSUM_SET


def field_fragment(dg: bytes, mtu: int, flags: int = 0):
    """Rule 5: the fragment that carries the L4 field of a datagram that gets one; None otherwise."""
    st, cnt, hlen, mx = fm.plan(dg, mtu, flags & TXF_FLAGS)
    proto = dg[9] if len(dg) >= 20 else None
    if not cnt or proto not in L4_FIELD or struct.unpack_from(">H", dg, 6)[0] & 0x3FFF:
        return None
    if len(dg) - hlen < L4_MIN[proto]:
        return None
    return L4_FIELD[proto] // mx if st & fm.FRAGMENTED else 0


def frames(fcs_oracle, inet_oracle, dg: bytes, mac: bytes, mtu: int, flags: int = fm.F_FCS):
    """txf_model.frames of the filled datagram; the status word carries the rule 4 bits."""
    filled, bits = fill(inet_oracle, dg, mtu, flags)
    st, out, crcs = fm.frames(fcs_oracle, inet_oracle, filled, mac, mtu, flags & TXF_FLAGS)
    return st | bits, out, crcs


def build(fcs_oracle, inet_oracle, dgram, off, ln, l2, mtu, flags, out, slot, slots, first=None, frames_fn=None):
    """txf_model.build with this module's frames. TXF_NO_ROOM datagrams keep only their protocol bits."""
    res = list(fm.build(fcs_oracle, inet_oracle, dgram, off, ln, l2, mtu, flags, out, slot, slots, first,
                        frames_fn or frames))
    status = res[3]
    for i in range(len(status)):
        if int(status[i]) & fm.NO_ROOM:
            status[i] = int(status[i]) & ~(L4_CSUM_SET | L4_SHORT)
    return tuple(res)
