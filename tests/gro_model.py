"""Expected-result model of one-pass RX coalescing: the rule list of include/nstack_gro.h, restated in
Python on top of tests/rxr_model.py (rules 1 and 5) and tests/rxd_model.py (rule 6). It parses with
`struct`, states rule 3 as the header states it (conditions (a)-(e) over sets, not a sorted walk),
takes every checksum from the oracle (oracle_ip_checksum, oracle_tcp_checksum) and has no arithmetic
of its own. Also the builder of TCP datagrams the tests cut and merge. Test infrastructure only."""
import json
import os
import struct

import numpy as np

import rxd_model as rd
import rxr_model as rr

CAND, MERGED, GFIN, GPSH = 0x1000, 0x2000, 0x4000, 0x8000
GROD_MERGED = 0x400
FIN, SYN, RST, PSH, ACK, URG, ECE, CWR = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
WIN_SHIFT, MAX_I = 15, 32768


def candidate(f: bytes, c):
    """Rule 2 for frame f with its rxr classification c: None, or dict(flow, seq, hlen, thl, P, tf, dg)."""
    st, hlen, I = c[:3]
    if not st & rr.WHOLE:
        return None
    dg = f[14:14 + I]
    L = I - hlen
    if dg[9] != 6 or L < 20 or I > MAX_I:
        return None
    thl = (dg[hlen + 12] >> 4) * 4
    if thl < 20 or thl > L or L - thl < 1 or dg[hlen + 13] & (SYN | RST | URG):
        return None
    return dict(flow=(dg[12:20], dg[hlen:hlen + 4]), seq=struct.unpack_from(">I", dg, hlen + 4)[0], hlen=hlen, thl=thl,
                P=L - thl, tf=dg[hlen + 13], dg=dg)


def _compared(x):
    """Rule 3d: the header bytes of a candidate with everything that may differ blanked."""
    hlen, thl = x["hlen"], x["thl"]
    h = bytearray(x["dg"][:hlen + thl])
    h[2:6] = bytes(4)
    h[10:12] = bytes(2)
    h[hlen + 4:hlen + 8] = bytes(4)
    h[hlen + 16:hlen + 18] = bytes(2)
    h[hlen + 13] &= ~(FIN | PSH | CWR) & 0xFF
    return bytes(h)


def coalescible(members, cand):
    """Rule 3 for a group (frame indices): (first, last) or None."""
    if len(members) < 2:
        return None
    seqs = [cand[i]["seq"] for i in members]
    starts = set(seqs)
    if len(starts) != len(seqs):                                                          # (a)
        return None
    end = {i: (cand[i]["seq"] + cand[i]["P"]) & 0xFFFFFFFF for i in members}
    lasts = [i for i in members if end[i] not in starts]                                  # (b)
    if len(lasts) != 1:
        return None
    first, last = min(members, key=lambda i: cand[i]["seq"]), lasts[0]
    if sum(cand[i]["P"] for i in members) != (end[last] - cand[first]["seq"]) & 0xFFFFFFFF:    # (c)
        return None
    ref = _compared(cand[first])
    for i in members:
        x = cand[i]
        if x["hlen"] != cand[first]["hlen"] or x["thl"] != cand[first]["thl"] or _compared(x) != ref:   # (d)
            return None
        if (i != last and x["tf"] & (FIN | PSH)) or (i != first and x["tf"] & CWR):      # (e)
            return None
    return first, last


def plan(frames, flags: int = 0, verdict=None, drop_mask: int = 0, align: int = 1, classify_fn=None):
    """rr.plan's dict with coalescing (rules 1-5 but for NO_ROOM and DELIVERED), plus "cand" and
    "merged": {first: [members in seq order]}."""
    base = rr.plan(frames, flags, verdict, drop_mask, align, classify_fn)
    n, cls, fstat = len(frames), base["cls"], base["fstat"].copy()
    cand = {}
    for i, f in enumerate(frames):
        x = candidate(f, cls[i])
        if x is not None:
            cand[i] = x
            fstat[i] |= CAND
    groups = {}
    for i, x in cand.items():
        groups.setdefault((x["flow"], x["seq"] >> WIN_SHIFT), []).append(i)
    # what rr.plan delivers, as head frames with their lengths and every frame's place behind its head
    D = {int(i): int(d) for i, d in zip(base["dlead"], base["dlen"])}
    headof = {i: int(base["dlead"][int(base["dgi"][i])]) for i in range(n) if base["dgi"][i] != rr.NONE32}
    rel = {i: int(base["dst"][i]) - int(base["doff"][int(base["dgi"][i])]) for i in headof}
    merged = {}
    for members in groups.values():
        fl = coalescible(members, cand)
        if fl is None:
            continue
        first, last = fl                                                                  # rule 4
        hb = cand[first]["hlen"] + cand[first]["thl"]
        fstat[members] |= MERGED
        fstat[first] |= rr.HEAD | (GFIN if cand[last]["tf"] & FIN else 0) | (GPSH if cand[last]["tf"] & PSH else 0)
        for i in members:
            if i != first:
                del D[i]
                headof[i] = first
                rel[i] = hb + ((cand[i]["seq"] - cand[first]["seq"]) & 0xFFFFFFFF)
        D[first] = hb + sum(cand[i]["P"] for i in members)
        merged[first] = sorted(members, key=lambda i: cand[i]["seq"])
    leads = sorted(D)                                                                     # rule 5
    doff = np.zeros(len(leads) + 1, dtype=np.uint64)
    dlen = np.array([D[i] for i in leads], dtype=np.uint32).reshape(len(leads))
    at = 0
    for k, i in enumerate(leads):
        doff[k] = at
        at += (D[i] + align - 1) & ~(align - 1)
    doff[len(leads)] = at
    k_of = {i: k for k, i in enumerate(leads)}
    dst = np.full(n, rr.NONE64, dtype=np.uint64)
    dgi = np.full(n, rr.NONE32, dtype=np.uint32)
    for i, h in headof.items():
        dgi[i] = k_of[h]
        dst[i] = int(doff[k_of[h]]) + rel[i]
    return dict(fstat=fstat, dst=dst, dgi=dgi, doff=doff, dlen=dlen, dlead=np.array(leads, dtype=np.uint32).reshape(len(leads)),
                m=len(leads), cls=cls, cand=cand, merged=merged)


def merged_datagram(inet_oracle, pl, first) -> bytes:
    """Rule 4: the bytes of the merged datagram whose first member is frame `first`."""
    cand, members = pl["cand"], pl["merged"][first]
    x, last = cand[first], cand[members[-1]]
    hlen, hb = x["hlen"], x["hlen"] + x["thl"]
    dg = bytearray(x["dg"][:hb])
    for i in members:
        y = cand[i]
        at = hb + ((y["seq"] - x["seq"]) & 0xFFFFFFFF)
        assert at == len(dg)                                                              # the members tile the range
        dg += y["dg"][hb:]
    struct.pack_into(">H", dg, 2, len(dg))
    dg[10:12] = b"\x00\x00"
    dg[10:12] = struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(dg[:hlen]), hlen))
    dg[hlen + 13] |= last["tf"] & (FIN | PSH)
    dg[hlen + 16:hlen + 18] = b"\x00\x00"
    src, dst = struct.unpack_from(">II", dg, 12)
    seg = bytes(dg[hlen:])
    dg[hlen + 16:hlen + 18] = struct.pack("<H", inet_oracle.oracle_tcp_checksum(src, dst, seg, len(seg)))
    return bytes(dg)


def build(inet_oracle, frames, pl, out, out_bytes=None):
    """(arena after the call, final status words): rr.build for everything that is not merged."""
    member = {i for ms in pl["merged"].values() for i in ms}
    rest = dict(pl)
    rest["dgi"] = pl["dgi"].copy()
    rest["dgi"][sorted(member)] = rr.NONE32
    arena, fstat = rr.build(inet_oracle, frames, rest, out, out_bytes)
    out_bytes = arena.size if out_bytes is None else out_bytes
    for first, members in pl["merged"].items():
        k = int(pl["dgi"][first])
        at, D = int(pl["doff"][k]), int(pl["dlen"][k])
        if at + D > out_bytes:
            fstat[members] |= rr.NO_ROOM
            continue
        dg = merged_datagram(inet_oracle, pl, first)
        assert len(dg) == D
        arena[at:at + D] = np.frombuffer(dg, dtype=np.uint8)
        fstat[members] |= rr.DELIVERED
    return arena, fstat


def verdicts(inet_oracle, out_bytes, pl, room=None) -> np.ndarray:
    """Rule 6: rd.verdicts, with GROD_MERGED | 6 << 16 on the merged datagrams that were written."""
    v = rd.verdicts(inet_oracle, out_bytes, pl, room)
    for first in pl["merged"]:
        k = int(pl["dgi"][first])
        if v[k] != rd.NO_ROOM:
            v[k] = GROD_MERGED | (6 << rd.PROTO_SHIFT)
    return v


# ---- TCP datagrams with the checksums the oracle computes ----
def tcp_datagram(inet_oracle, payload: bytes, seq: int, hlen=20, thl=20, tflags=ACK, src=0x0A000001, dst=0x0A000002,
                 sport=0x8001, dport=0x0050, ack=0x0A0B0C0D, window=0x2000, ident=0x1234, ttl=64, tos=0, foff=0,
                 ipopt=None, tcpopt=None) -> bytes:
    ipopt = bytes(range(1, hlen - 19)) if ipopt is None else ipopt
    tcpopt = bytes(range(0x41, 0x41 + thl - 20)) if tcpopt is None else tcpopt
    assert len(ipopt) == hlen - 20 and len(tcpopt) == thl - 20
    seg = bytearray(struct.pack(">HHIIBBHHH", sport, dport, seq & 0xFFFFFFFF, ack, (thl // 4) << 4, tflags, window, 0, 0) +
                    tcpopt + payload)
    seg[16:18] = struct.pack("<H", inet_oracle.oracle_tcp_checksum(src, dst, bytes(seg), len(seg)))
    h = bytearray(struct.pack(">BBHHHBBHII", 0x40 | hlen // 4, tos, hlen + len(seg), ident, foff, ttl, 6, 0, src, dst) + ipopt)
    h[10:12] = struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(h), hlen))
    return bytes(h) + bytes(seg)


def load_golden():
    """The fixtures of tests/golden/make_gro_golden.py: per case its frames and expected datagrams as bytes."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "gro_vectors.json")) as f:
        vec = json.load(f)
    with open(os.path.join(golden, vec["arena"]), "rb") as f:
        blob = f.read()
    for c in vec["cases"]:
        at, c["frames"] = c["at"], []
        for F in c["flen"]:
            c["frames"].append(blob[at:at + F])
            at += F
        assert at == c["dat"]
        c["dgrams"] = []
        for D in c["dlen"]:
            c["dgrams"].append(blob[at:at + D])
            at += D
    return vec
