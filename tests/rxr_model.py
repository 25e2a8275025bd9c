"""Expected-result model of one-pass RX reassembly: the rule list of include/nstack_rxr.h, restated
in Python. It parses with `struct`, states rule 6 as the header states it (the five conditions, not
a sorted walk), takes the header checksum from the oracle (oracle_ip_checksum) and has no arithmetic
of its own. Test infrastructure only."""
import json
import os
import struct

import numpy as np

F_TRAILER = 1
WHOLE, FRAG, HEAD, DROPPED, NOT_IPV4, BAD_HDR = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
BAD_LEN, FRAG_BAD, INCOMPLETE, TOO_BIG, NO_ROOM, DELIVERED = 0x040, 0x080, 0x100, 0x200, 0x400, 0x800
NONE32, NONE64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF


def classify(f: bytes, flags: int = 0, dropped: bool = False):
    """Rules 1-5: (status, hlen, I, o, L, mf, key)."""
    T = 4 if flags & F_TRAILER else 0
    if dropped:                                                          # rule 1
        return DROPPED, 0, 0, 0, 0, False, None
    F = len(f)
    if F < 14 + T or struct.unpack_from(">H", f, 12)[0] != 0x0800:       # rule 2
        return NOT_IPV4, 0, 0, 0, 0, False, None
    P = F - 14 - T
    if P < 20:
        return BAD_HDR, 0, 0, 0, 0, False, None
    vhl, _tos, I, ident, foff, _ttl, proto = struct.unpack_from(">BBHHHBB", f, 14)
    hlen = (vhl & 0x0F) * 4
    if (vhl & 0x40) != 0x40 or hlen < 20 or hlen > P:
        return BAD_HDR, 0, 0, 0, 0, False, None
    if I < hlen or I > P:                                                # rule 3
        return BAD_LEN, hlen, I, 0, 0, False, None
    if foff & 0x3FFF == 0:                                               # rule 4
        return WHOLE, hlen, I, 0, 0, False, None
    o, L, mf = (foff & 0x1FFF) * 8, I - hlen, bool(foff & 0x2000)        # rule 5
    st = FRAG
    if L == 0 or o + L + 20 > 65535:
        st |= FRAG_BAD
    elif o == 0:
        st |= HEAD
    return st, hlen, I, o, L, mf, (f[26:34], proto, ident)              # rule 6: src, dst, proto, id


def plan(frames, flags: int = 0, verdict=None, drop_mask: int = 0, align: int = 1, classify_fn=None):
    """The plan arrays of a batch (rules 1-8 but for NO_ROOM and DELIVERED), as a dict of numpy arrays
    plus "m" and, for build(), "cls". classify_fn: a caller's memoised `classify`."""
    cf = classify_fn or classify
    n = len(frames)
    cls = [cf(f, flags, bool(verdict is not None and int(verdict[i]) & drop_mask)) for i, f in enumerate(frames)]
    fstat = np.array([c[0] for c in cls], dtype=np.uint32).reshape(n)
    groups = {}
    for i, c in enumerate(cls):
        if c[0] & FRAG and not c[0] & FRAG_BAD:
            groups.setdefault(c[6], []).append(i)
    D, headof, rel = {}, {}, {}
    for i, c in enumerate(cls):
        if c[0] & WHOLE:
            D[i], headof[i], rel[i] = c[2], i, 0
    for members in groups.values():
        heads = [i for i in members if cls[i][3] == 0]
        lasts = [i for i in members if not cls[i][5]]
        offs = [cls[i][3] for i in members]
        starts = set(offs)
        complete = (len(heads) == 1 and len(lasts) == 1 and len(starts) == len(offs)
                    and all(cls[i][3] + cls[i][4] in starts for i in members if cls[i][5])
                    and sum(cls[i][4] for i in members) == cls[lasts[0]][3] + cls[lasts[0]][4])
        if not complete:
            fstat[members] |= INCOMPLETE
            continue
        h, total = heads[0], cls[lasts[0]][3] + cls[lasts[0]][4]
        if cls[h][1] + total > 65535:
            fstat[members] |= TOO_BIG
            continue
        D[h] = cls[h][1] + total                                         # rule 7
        for i in members:
            headof[i] = h
            rel[i] = cls[h][1] + cls[i][3] if cls[i][3] else 0
    leads = sorted(D)                                                    # rule 8
    doff = np.zeros(len(leads) + 1, dtype=np.uint64)
    dlen = np.array([D[i] for i in leads], dtype=np.uint32).reshape(len(leads))
    at = 0
    for k, i in enumerate(leads):
        doff[k] = at
        at += (D[i] + align - 1) & ~(align - 1)
    doff[len(leads)] = at
    k_of = {i: k for k, i in enumerate(leads)}
    dst = np.full(n, NONE64, dtype=np.uint64)
    dgi = np.full(n, NONE32, dtype=np.uint32)
    for i, h in headof.items():
        dgi[i] = k_of[h]
        dst[i] = int(doff[k_of[h]]) + rel[i]
    return dict(fstat=fstat, dst=dst, dgi=dgi, doff=doff, dlen=dlen, dlead=np.array(leads, dtype=np.uint32).reshape(len(leads)),
                m=len(leads), cls=cls)


def build(inet_oracle, frames, pl, out, out_bytes=None):
    """(arena after the call, final status words). `out` is the arena before the call (a uint8 array:
    its content survives outside delivered datagrams)."""
    arena = np.array(out, dtype=np.uint8, copy=True)
    out_bytes = arena.size if out_bytes is None else out_bytes
    fstat = pl["fstat"].copy()
    for i, f in enumerate(frames):
        if pl["dgi"][i] == NONE32:
            continue
        k = int(pl["dgi"][i])
        if int(pl["doff"][k]) + int(pl["dlen"][k]) > out_bytes:          # rule 8
            fstat[i] |= NO_ROOM
            continue
        st, hlen, I = pl["cls"][i][:3]
        if st & WHOLE:
            piece = f[14:14 + I]
        elif st & HEAD:                                                  # rule 7
            hdr = bytearray(f[14:14 + hlen])
            struct.pack_into(">H", hdr, 2, int(pl["dlen"][k]))
            hdr[6:8] = b"\x00\x00"
            hdr[10:12] = b"\x00\x00"
            hdr[10:12] = struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(hdr), hlen))
            piece = bytes(hdr) + f[14 + hlen:14 + I]
        else:
            piece = f[14 + hlen:14 + I]
        at = int(pl["dst"][i])
        arena[at:at + len(piece)] = np.frombuffer(piece, dtype=np.uint8)
        fstat[i] |= DELIVERED
    return arena, fstat


def datagrams(arena, pl):
    """The delivered datagrams of an arena, as bytes, in datagram order."""
    return [arena[int(pl["doff"][k]):int(pl["doff"][k]) + int(pl["dlen"][k])].tobytes() for k in range(pl["m"])]


def layout(frames, lead: int = 0, gap: int = 0, fill: int = 0xEE, order=None):
    """(arena, off, len): the frames back to back with `gap` bytes between them, `lead` bytes in front;
    order: the frames' places in the arena (a permutation), frame i staying frame i."""
    n = len(frames)
    place = list(range(n)) if order is None else list(order)
    off = np.zeros(n, dtype=np.uint64)
    ln = np.array([len(f) for f in frames], dtype=np.uint32).reshape(n)
    at = lead
    for i in sorted(range(n), key=lambda q: place[q]):
        off[i] = at
        at += len(frames[i]) + gap
    arena = np.full(max(at - gap if n else lead, 1), fill, dtype=np.uint8)
    for i, f in enumerate(frames):
        arena[int(off[i]):int(off[i]) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    return arena, off, ln


def load_golden():
    """The fixtures of tests/golden/make_rxr_golden.py: per case its frames and expected datagrams as bytes."""
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(golden, "rxr_vectors.json")) as f:
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
