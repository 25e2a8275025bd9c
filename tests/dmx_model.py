"""Expected-result model of one-pass RX demultiplexing: the rule list of include/nstack_dmx.h restated
over Python dicts and per-socket lists, for datagrams as tests/rxd_model.py and tests/gro_model.py
build them. It parses with `struct` and has no arithmetic of its own beyond the record layout
(struct nstack_dgram on LP64 and the round-up to `align`). Test infrastructure only."""
import json
import os
import struct

import numpy as np

import rxd_model as rd

DROPPED, NO_PROTO, SHORT, CTRL, NO_SOCK, QUEUED, NO_ROOM, DELIVERED = 0x01, 0x02, 0x04, 0x08, 0x10, 0x20, 0x40, 0x80
NONE32, NONE64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
REC_HDR = 24
SYN, RST = 0x02, 0x04
MAX_SOCKS = 65536


def key(proto: int, port: int, addr: int) -> int:
    return (proto << 48) | (port << 32) | addr


def key_valid(k: int) -> bool:
    return (k >> 48) in (6, 17)


def parse(dg: bytes):
    """Rules 1 (the length part) to 4 for one datagram: (status, None) or (0 | CTRL, fields)."""
    D = len(dg)
    if D < 20:
        return DROPPED, None
    hlen = (dg[0] & 15) * 4
    if not 20 <= hlen <= D:
        return DROPPED, None
    proto = dg[9]
    if proto not in (6, 17):
        return NO_PROTO, None                                             # rule 2
    seg = dg[hlen:]
    L, st = len(seg), 0
    if proto == 17:                                                       # rule 3
        if L < 8:
            return SHORT, None
        pay = seg[8:]
    else:                                                                 # rule 4
        if L < 20:
            return SHORT, None
        thl = (seg[12] >> 4) * 4
        if not 20 <= thl <= L:
            return SHORT, None
        pay = seg[thl:]
        if len(pay) == 0 or seg[13] & (SYN | RST):
            st = CTRL
    src, dst = struct.unpack_from(">II", dg, 12)
    sport, dport = struct.unpack_from(">HH", seg, 0)
    return st, dict(proto=proto, src=src, dst=dst, sport=sport, dport=dport, pay=bytes(pay))


def record(f, align: int) -> bytes:
    """Rule 6: struct nstack_dgram { {u32 addr, int port} src, dst; size_t buf_size; buf[] }, padded with zeros."""
    r = struct.pack("<IiIiQ", f["src"], f["sport"], f["dst"], f["dport"], len(f["pay"])) + f["pay"]
    return r + bytes(-len(r) % align)


def plan(out, out_bytes, doff, dlen, bind, align=8, dverdict=None, drop_mask=0, n=None):
    """The plan of the m = len(doff) datagrams in the uint8 array `out`; n: the arrays' capacity."""
    m = len(doff)
    n = m if n is None else n
    S = len(bind)
    assert S <= MAX_SOCKS and align in (8, 16, 32, 64, 128) and n >= m
    lowest = {}
    for s, k in enumerate(bind):
        if key_valid(int(k)):
            lowest.setdefault(int(k), s)                                  # a key belongs to its lowest index
    dstat, dsock = np.zeros(n, np.uint32), np.full(n, NONE32, np.uint32)
    rec = np.full(n, NONE64, np.uint64)
    queues = [[] for _ in range(S)]                                       # (k, record) in ascending k
    fields = [None] * m
    for k in range(m):
        at, D = int(doff[k]), int(dlen[k])
        if at + D > out_bytes or (dverdict is not None and int(dverdict[k]) & (drop_mask | rd.NO_ROOM)):
            dstat[k] = DROPPED                                            # rule 1
            continue
        st, f = parse(bytes(out[at:at + D]))
        if f is not None:                                                 # rule 5
            s = lowest.get(key(f["proto"], f["dport"], f["dst"]))
            if s is None:
                st |= NO_SOCK
            else:
                dsock[k] = s
            if st == 0:
                st = QUEUED
                queues[s].append((k, record(f, align)))
                fields[k] = f
        dstat[k] = st
    sbase, scnt = np.zeros(S + 1, np.uint64), np.zeros(S, np.uint32)
    recs = {}
    at = 0
    for s, qd in enumerate(queues):                                       # rule 7
        sbase[s], scnt[s] = at, len(qd)
        for k, r in qd:
            rec[k] = at
            recs[k] = r
            at += len(r)
    sbase[S] = at
    qcounts = np.array([len(recs), at, int(((dstat & NO_SOCK) != 0).sum()), int(((dstat & DROPPED) != 0).sum())], np.uint64)
    return dict(m=m, n=n, S=S, align=align, dstat=dstat, dsock=dsock, rec=rec, sbase=sbase, scnt=scnt, qcounts=qcounts,
                recs=recs, fields=fields)


def build(pl, q, q_bytes=None):
    """Rule 8: writes the records that have room into the uint8 array q; returns the final words."""
    q_bytes = len(q) if q_bytes is None else q_bytes
    fin = pl["dstat"].copy()
    for k, r in pl["recs"].items():
        at = int(pl["rec"][k])
        if at + len(r) > q_bytes:
            fin[k] |= NO_ROOM
        else:
            q[at:at + len(r)] = np.frombuffer(r, np.uint8)
            fin[k] |= DELIVERED
    return fin


def queue_of(pl, q, s):
    """The records of socket s as the reference's nstack_recvfrom would walk them: [(src, sport, payload)]."""
    out, at = [], int(pl["sbase"][s])
    for _ in range(int(pl["scnt"][s])):
        src, sport, dst, dport, size = struct.unpack_from("<IiIiQ", q, at)
        out.append((src, sport, dst, dport, bytes(q[at + REC_HDR:at + REC_HDR + size])))
        at += -(-(REC_HDR + size) // pl["align"]) * pl["align"]
    assert at == int(pl["sbase"][s + 1])
    return out


# ---- datagram builders (checksum fields are not looked at by these rules) ----
def ip_datagram(proto: int, seg: bytes, src=0x0A000001, dst=0x0A000002, hlen=20, ident=1) -> bytes:
    opts = bytes([1] * (hlen - 20))
    return struct.pack(">BBHHHBBHII", 0x40 | (hlen // 4), 0, hlen + len(seg), ident, 0, 64, proto, 0, src, dst) + opts + seg


def udp(payload: bytes, dport: int, sport=0x1234, **kw) -> bytes:
    return ip_datagram(17, struct.pack(">HHHH", sport, dport, 8 + len(payload), 0) + payload, **kw)


def tcp(payload: bytes, dport: int, sport=0x8001, thl=20, tflags=0x18, seq=1, **kw) -> bytes:
    seg = struct.pack(">HHIIBBHHH", sport, dport, seq, 2, (thl // 4) << 4, tflags, 0x2000, 0, 0) + bytes([1] * (thl - 20))
    return ip_datagram(6, seg + payload, **kw)


def load_golden():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(here, "dmx_vectors.json")) as f:
        vec = json.load(f)
    blob = np.fromfile(os.path.join(here, vec["blob"]), dtype=np.uint8)
    return vec, blob
