"""Expected-verdict model of reassembly with L4 verdicts: the rule list of include/nstack_rxd.h,
restated in Python and applied to the datagrams tests/rxr_model.py builds. It parses with `struct`,
takes every checksum from the oracle (oracle_tcp_checksum, oracle_udp_checksum, oracle_ip_checksum)
and has no arithmetic of its own. Also the builders of L4 segments whose checksum field the oracle
filled. Test infrastructure only."""
import socket
import struct

import numpy as np

NO_ROOM, L4_CHECKED, L4_BAD_CSUM, L4_SHORT = 0x002, 0x080, 0x100, 0x200
PROTO_SHIFT = 16
L4_BITS = L4_CHECKED | L4_BAD_CSUM | L4_SHORT | (0xFF << PROTO_SHIFT)
PROTO = {"tcp": 6, "udp": 17, "icmp": 1}


def verdict(inet_oracle, dg: bytes) -> int:
    """Rules 2 and 3: the verdict word of one delivered datagram."""
    D = len(dg)
    hlen, proto = (dg[0] & 0x0F) * 4, dg[9]
    src_raw, dst_raw = struct.unpack_from("<II", dg, 12)                 # the address words as they lie
    L = D - hlen
    seg = dg[hlen:]
    v = proto << PROTO_SHIFT
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
        v |= L4_CHECKED | (L4_BAD_CSUM if bad else 0)
    return v


def verdicts(inet_oracle, out_bytes, plan, room=None) -> np.ndarray:
    """The verdict words of the plan's m datagrams. out_bytes: the output arena after the build
    (rxr_model.build), a uint8 array; room: the capacity the build was given (default: the arena)."""
    arena = np.asarray(out_bytes, dtype=np.uint8)
    room = arena.size if room is None else room
    v = np.zeros(plan["m"], dtype=np.uint32)
    for k in range(plan["m"]):
        at, D = int(plan["doff"][k]), int(plan["dlen"][k])
        v[k] = NO_ROOM if at + D > room else verdict(inet_oracle, arena[at:at + D].tobytes())   # rule 1
    return v


def count_bad(v, bad_mask: int) -> int:
    return int(((np.asarray(v, dtype=np.uint32) & np.uint32(bad_mask)) != 0).sum())


# ---- L4 segments with the checksum the oracle computes (src, dst: host-order ints, as make_rxr_golden.ip_packet takes them) ----
def _raw(addr: int) -> int:
    return struct.unpack("<I", struct.pack(">I", addr))[0]


def udp_segment(inet_oracle, payload: bytes, src: int, dst: int, sport=0x1234, dport=0x0035) -> bytes:
    seg = bytearray(struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload)
    c = inet_oracle.oracle_udp_checksum(bytes(seg), len(seg), _raw(src), _raw(dst))
    seg[6:8] = struct.pack("<H", c if c else 0xFFFF)                     # src/udp.c: a computed zero goes out as 0xffff
    return bytes(seg)


def tcp_segment(inet_oracle, payload: bytes, src: int, dst: int, sport=0x8001, dport=0x0050) -> bytes:
    seg = bytearray(struct.pack(">HHIIHHHH", sport, dport, 0x01020304, 0x0A0B0C0D, 0x5018, 0x2000, 0, 0) + payload)
    seg[16:18] = struct.pack("<H", inet_oracle.oracle_tcp_checksum(src, dst, bytes(seg), len(seg)))
    return bytes(seg)


def icmp_segment(inet_oracle, payload: bytes, *_addr) -> bytes:
    seg = bytearray(struct.pack(">BBHHH", 8, 0, 0, 0x0102, 0x0304) + payload)
    seg[2:4] = struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(seg), len(seg)))
    return bytes(seg)


SEGMENT = {"udp": udp_segment, "tcp": tcp_segment, "icmp": icmp_segment}


def segment(inet_oracle, kind: str, payload: bytes, src: int, dst: int) -> bytes:
    """A `kind` segment around `payload` whose checksum the reference's own function accepts."""
    seg = SEGMENT[kind](inet_oracle, payload, src, dst)
    assert verdict(inet_oracle, struct.pack(">BBHHHBBHII", 0x45, 0, 20 + len(seg), 0, 0, 64, PROTO[kind], 0, src, dst) + seg) == \
        (PROTO[kind] << PROTO_SHIFT) | L4_CHECKED, kind
    return seg
