"""Expected-result model of one-pass TX framing: the rule list of include/nstack_txf.h, restated
in Python. It parses and builds with `struct`, takes every CRC and checksum from the oracle
(oracle_ether_fcs, oracle_ip_checksum) and has no arithmetic of its own. Test infrastructure only."""
import json
import os
import struct

import numpy as np

F_FCS, F_HONOR_DF, F_L2_ONE = 1, 2, 4
WHOLE, FRAGMENTED, BAD_HDR, BAD_LEN, REFRAG, DF_DROP, NO_ROOM = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020, 0x040
L2_DTYPE = np.dtype([("dst", "u1", (6,)), ("src", "u1", (6,))])


def frag_unit(mtu: int, hlen: int) -> int:
    return (mtu - hlen - 8 + 7) & ~7                                     # rule 6 (ip.c:220-233)


def min_slot(mtu: int, flags: int) -> int:
    return max(14 + mtu, 70) + (4 if flags & F_FCS else 0)               # rule 9


def plan(dg: bytes, mtu: int, flags: int = 0):
    """(status, cnt, hlen, max) of one datagram: rules 1-6."""
    D = len(dg)
    if D < 20:                                                           # rule 1
        return BAD_HDR, 0, 0, 0
    vhl, _tos, ip_len, _id, foff = struct.unpack_from(">BBHHH", dg, 0)
    hlen = (vhl & 0x0F) * 4
    if (vhl & 0x40) != 0x40 or hlen < 20 or hlen > D:
        return BAD_HDR, 0, 0, 0
    if ip_len != D:                                                      # rule 2
        return BAD_LEN, 0, hlen, 0
    if D <= mtu:                                                         # rule 3
        return WHOLE, 1, hlen, 0
    st = 0
    if foff & 0x3FFF:                                                    # rule 4
        st |= REFRAG
    if flags & F_HONOR_DF and foff & 0x4000:                             # rule 5
        st |= DF_DROP
    if st:
        return st, 0, hlen, 0
    mx = frag_unit(mtu, hlen)                                            # rule 6
    return FRAGMENTED, -(-(D - hlen) // mx), hlen, mx


def frames(fcs_oracle, inet_oracle, dg: bytes, mac: bytes, mtu: int, flags: int = F_FCS):
    """(status, [frame bytes: F, plus the 4 FCS bytes with F_FCS], [fcs values, 0 without F_FCS])."""
    st, cnt, hlen, mx = plan(dg, mtu, flags)
    out, crcs = [], []
    for j in range(cnt):
        hdr = bytearray(dg[:hlen])
        if st & WHOLE:
            pay = dg[hlen:]
        else:
            pay = dg[hlen + j * mx:hlen + (j + 1) * mx]
            struct.pack_into(">H", hdr, 2, hlen + len(pay))
            struct.pack_into(">H", hdr, 6, (0x2000 if j < cnt - 1 else 0) | (j * mx >> 3))
        hdr[10:12] = b"\x00\x00"                                         # rule 7
        hdr[10:12] = struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(hdr), hlen))
        ip = bytes(hdr) + pay
        body = bytes(mac[:12]) + b"\x08\x00" + ip + bytes(max(0, 56 - len(ip)))   # rule 8
        fcs = 0
        if flags & F_FCS:
            fcs = fcs_oracle.oracle_ether_fcs(body, len(body))
            body += struct.pack("<I", fcs)
        out.append(body)
        crcs.append(fcs)
    return st, out, crcs


def build(fcs_oracle, inet_oracle, dgram, off, ln, l2, mtu, flags, out, slot, slots, first=None, frames_fn=None):
    """A batch: (arena after the call, flen, fcs, status, first). `out` is the arena before the call
    (a uint8 array: its content survives outside produced frames), l2 an (n, 12) or L2_DTYPE array;
    first = None packs the frames (the plan call's prefix sums). flen and fcs start as 0xCCCCCCCC
    and hold values for produced frames only. frames_fn: a caller's memoised `frames`."""
    frames_fn = frames_fn or frames
    buf = dgram.tobytes() if isinstance(dgram, np.ndarray) else bytes(dgram)
    macs = np.ascontiguousarray(l2).view(np.uint8).reshape(-1, 12)
    n = len(off)
    arena = np.array(out, dtype=np.uint8, copy=True)
    flen = np.full(slots, 0xCCCCCCCC, dtype=np.uint32)
    fcs = np.full(slots, 0xCCCCCCCC, dtype=np.uint32)
    status = np.zeros(n, dtype=np.uint32)
    plan_first = np.zeros(n + 1, dtype=np.uint64)
    k = 0
    for i in range(n):
        dg = buf[int(off[i]):int(off[i]) + int(ln[i])]
        mac = macs[0 if flags & F_L2_ONE else i].tobytes()
        st, fr, crcs = frames_fn(fcs_oracle, inet_oracle, dg, mac, mtu, flags)
        plan_first[i] = k
        k0 = k if first is None else int(first[i])
        k += len(fr)
        if fr and k0 + len(fr) > slots:                                  # rule 9
            st |= NO_ROOM
            fr = []
        status[i] = st
        for q, body in enumerate(fr):
            at = (k0 + q) * slot
            arena[at:at + len(body)] = np.frombuffer(body, dtype=np.uint8)
            flen[k0 + q] = len(body) - (4 if flags & F_FCS else 0)
            fcs[k0 + q] = crcs[q]
    plan_first[n] = k
    return arena, flen, fcs, status, plan_first


def load_golden():
    """The fixtures of tests/golden/make_txf_golden.py: the records, the input bytes, the frames per mtu."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "txf_vectors.json")) as f:
        vec = json.load(f)
    with open(os.path.join(golden, vec["input"]), "rb") as f:
        vec["input_bytes"] = f.read()
    vec["frame_bytes"] = {}
    for mtu, name in vec["frames"].items():
        with open(os.path.join(golden, name), "rb") as f:
            vec["frame_bytes"][int(mtu)] = f.read()
    return vec
