"""Generate the RX-reassembly fixtures (tests/golden/rxr_vectors.{bin,json}).

    python tests/golden/make_rxr_golden.py

Batches of frames and what include/nstack_rxr.h says becomes of them, from an INDEPENDENT formulation
written only for this script: frames are parsed by slicing, the fragments of a key are sorted by
offset and walked once (an exact tiling starts at 0, every piece starts where the one before ended,
every piece but the last has MF), and the header checksum is RFC 1071 over big-endian 16-bit words as
in make_rxv_golden.py. It uses neither the oracle nor the model (tests/rxr_model.py), and nothing of
the reference: its reassembly (src/ip_fragment.c) computes another ip_len and overwrites on overlap,
so no output of it could back these vectors. tests/test_rxr_model.py checks the model and the host
plan against them, tests/test_gpu_rxr.py the kernels. The frame builders also serve those tests.

A case is one batch. The .bin holds every case's frames back to back and then its expected datagrams
back to back; the .json their lengths, the call's arguments and the expected status words.
Totals of 1 and 8 payload bytes exist as whole datagrams only: a fragment group needs a head with MF
whose end is a multiple of 8 and a successor of at least one byte, so its smallest total is 9.
"""
import json
import os
import random
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))

F_TRAILER = 1
WHOLE, FRAG, HEAD, DROPPED, NOT_IPV4, BAD_HDR = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
BAD_LEN, FRAG_BAD, INCOMPLETE, TOO_BIG, NO_ROOM, DELIVERED = 0x040, 0x080, 0x100, 0x200, 0x400, 0x800
MF = 0x2000


def be_csum(b: bytes) -> int:
    s = sum(struct.unpack(f">{len(b) // 2}H", b))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return ~s & 0xFFFF


# ---- builders ----
def ip_packet(payload: bytes, hlen=20, foff=0, ident=0x1234, src=0x0A000001, dst=0x0A000002, proto=17, ip_len=None,
              vhl=None, rng=None) -> bytes:
    opts = bytes(rng.randrange(256) for _ in range(hlen - 20)) if rng else bytes(hlen - 20)
    h = bytearray(struct.pack(">BBHHHBBHII", (0x40 | hlen // 4) if vhl is None else vhl, 0,
                              hlen + len(payload) if ip_len is None else ip_len, ident, foff, 64, proto, 0, src, dst) + opts)
    h[10:12] = struct.pack(">H", be_csum(bytes(h)))
    return bytes(h) + payload


def frame(ip: bytes, trailer: bool, etype=0x0800, pad=46, mac=None) -> bytes:
    """An Ethernet frame around `ip`: zero padding up to `pad` payload bytes, the FCS with `trailer`."""
    body = (mac or bytes(range(1, 13))) + struct.pack(">H", etype) + ip + bytes(max(0, pad - len(ip)))
    return body + struct.pack("<I", zlib.crc32(body)) if trailer else body


def fragments(rng, payload: bytes, cuts, trailer, hlen_head=20, hlen_rest=20, **kw):
    """The frames of `payload` cut at the byte offsets `cuts` (multiples of 8), in offset order."""
    edges = [0] + list(cuts) + [len(payload)]
    out = []
    for q in range(len(edges) - 1):
        a, e = edges[q], edges[q + 1]
        foff = (a >> 3) | (MF if q < len(edges) - 2 else 0)
        out.append(frame(ip_packet(payload[a:e], hlen_head if q == 0 else hlen_rest, foff=foff, rng=rng, **kw), trailer))
    return out


# ---- the expected result, by slicing and one sorted walk ----
def expect(frames, flags, verdict=None, drop_mask=0, out_bytes=None, align=1):
    """(status words, [(lead, datagram bytes)])."""
    T = 4 if flags & F_TRAILER else 0
    st = [0] * len(frames)
    groups, whole = {}, {}
    for i, f in enumerate(frames):
        if verdict is not None and verdict[i] & drop_mask:
            st[i] = DROPPED
            continue
        if len(f) < 14 + T or f[12:14] != b"\x08\x00":
            st[i] = NOT_IPV4
            continue
        ip = f[14:len(f) - T]
        hlen = (ip[0] & 15) * 4 if ip else 0
        if len(ip) < 20 or ip[0] & 0x40 != 0x40 or hlen < 20 or hlen > len(ip):
            st[i] = BAD_HDR
            continue
        ip_len = int.from_bytes(ip[2:4], "big")
        if ip_len < hlen or ip_len > len(ip):
            st[i] = BAD_LEN
            continue
        ip = ip[:ip_len]
        foff = int.from_bytes(ip[6:8], "big")
        if foff & 0x3FFF == 0:
            st[i] = WHOLE
            whole[i] = ip
            continue
        st[i] = FRAG
        o, pay = (foff & 0x1FFF) * 8, ip[hlen:]
        if not pay or o + len(pay) + 20 > 65535:
            st[i] |= FRAG_BAD
            continue
        if o == 0:
            st[i] |= HEAD
        groups.setdefault(ip[12:20] + ip[9:10] + ip[4:6], []).append((o, i, pay, bool(foff & MF), ip[:hlen]))
    made = dict(whole)
    for g in groups.values():
        g.sort()
        pos, ok = 0, True
        for q, (o, i, pay, mf, _h) in enumerate(g):
            ok = ok and o == pos and mf == (q < len(g) - 1)
            pos += len(pay)
        hdr = bytearray(g[0][4])
        if ok and len(hdr) + pos > 65535:
            for _o, i, *_ in g:
                st[i] |= TOO_BIG
        elif ok:
            hdr[2:4] = struct.pack(">H", len(hdr) + pos)
            hdr[6:8] = b"\x00\x00"
            hdr[10:12] = b"\x00\x00"
            hdr[10:12] = struct.pack(">H", be_csum(bytes(hdr)))
            made[g[0][1]] = bytes(hdr) + b"".join(p for _o, _i, p, _m, _h in g)
            for _o, i, *_ in g:
                st[i] |= 0x10000 | (g[0][1] << 20)   # scratch: member of the datagram led by g[0][1]
        else:
            for _o, i, *_ in g:
                st[i] |= INCOMPLETE
    out, at = [], 0
    fate = {}
    for lead in sorted(made):
        D = len(made[lead])
        fits = out_bytes is None or at + D <= out_bytes
        fate[lead] = DELIVERED if fits else NO_ROOM
        out.append((lead, made[lead], fits))
        at += (D + align - 1) & ~(align - 1)
    for i in range(len(frames)):
        if st[i] & 0x10000:
            lead = st[i] >> 20
            st[i] = (st[i] & 0xFFFF) | fate[lead]
        elif st[i] & WHOLE:
            st[i] |= fate[i]
    return st, out


# ---- the cases ----
def cases():
    rng = random.Random(20260406)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    C = []

    def add(tag, frames, flags=0, **kw):
        C.append(dict(tag=tag, frames=frames, flags=flags, **kw))

    for t in (0, 1):
        tr, sfx = bool(t), f"_t{t}"
        # whole datagrams: every header length, payloads of 0, 1, 8 and more, padded and not
        add("whole_hlens" + sfx, [frame(ip_packet(rb(n), hl, ident=hl, rng=rng), tr)
                                  for hl in range(20, 64, 4) for n in (0, 1, 8, 25, 26, 27, 300)], t)
        # one frame per status bit, a good datagram before, between and behind
        good = lambda k: frame(ip_packet(rb(40 + k), ident=0x7000 + k), tr)
        too_big = fragments(rng, rb(65515), [65512 - 8 * 40, 65512], tr, hlen_head=60, hlen_rest=20, ident=0x7777)
        bits = [good(0),
                frame(rb(28), tr, etype=0x0806),                                   # ARP
                frame(b"\x00\x05\x08\x00" + ip_packet(rb(30)), tr, etype=0x8100),  # VLAN
                frame(b"\x60" + rb(59), tr, etype=0x86DD),                         # IPv6
                rb(13 + 4 * t),                                                    # runt
                good(1),
                frame(ip_packet(rb(30), vhl=0x25), tr),                            # bad version bit
                frame(ip_packet(rb(30), vhl=0x44), tr),                            # hlen 16
                frame(ip_packet(rb(4), hlen=20, vhl=0x4F), tr, pad=0),             # hlen 60 > P
                frame(rb(19), tr, pad=0),                                          # P < 20
                frame(ip_packet(rb(30), ip_len=19), tr),                           # ip_len < hlen
                frame(ip_packet(rb(30), ip_len=51), tr, pad=0),                    # ip_len > P
                frame(ip_packet(rb(10), ip_len=30), tr),                           # ip_len == P - 16: padding
                frame(ip_packet(rb(100), ip_len=60), tr),                          # ip_len below P: tail stripped
                good(2),
                frame(ip_packet(b"", foff=MF | 2, ident=0x7100), tr),              # L == 0
                frame(ip_packet(rb(8), foff=65528 >> 3, ident=0x7101), tr),        # o = 65528: too far
                frame(ip_packet(rb(16), foff=MF, ident=0x7102), tr),               # a lone head
                frame(ip_packet(rb(16), foff=3, ident=0x7103), tr),                # a lone last
                ] + too_big + [good(3)]
        verdict = [0] * len(bits)
        verdict[5] = 0x21   # FCS_BAD | IP_BAD_CSUM, as the validator would say
        verdict[0] = 0x40   # a bit outside the mask
        add("status_bits" + sfx, bits, t, verdict=verdict, drop_mask=0x3B)
        add("no_room" + sfx, [good(4)] + fragments(rng, rb(100), [48], tr, ident=0x7200) + [good(5)], t, out_bytes=164)
        # header lengths on head and non-head differ
        fr = []
        for q, (hh, hr) in enumerate(((20, 60), (60, 20), (24, 28), (44, 20), (20, 24), (56, 60))):
            fr += fragments(rng, rb(200 + q), [64, 128], tr, hlen_head=hh, hlen_rest=hr, ident=0x100 + q)
        add("hlens_differ" + sfx, fr, t)
        # last fragments of 1..8 bytes in padded frames; totals 9 and 16
        fr = []
        for tl in range(1, 9):
            fr += fragments(rng, rb(8 + tl), [8], tr, ident=0x200 + tl)
            fr += fragments(rng, rb(1472 + tl), [1472], tr, ident=0x300 + tl, hlen_head=24)
        add("short_lasts" + sfx, fr, t)
        # what cannot be completed
        p = rb(96)
        full = lambda ident, **kw: fragments(rng, p, [32, 64], tr, ident=ident, **kw)
        fr = good(6), *full(0x400)[1:], *full(0x401)[::2], *full(0x402)[:2], good(7)          # no head, middle, last
        two_lasts = full(0x403) + [frame(ip_packet(rb(8), foff=96 >> 3, ident=0x403), tr)]
        dup = full(0x404) + [full(0x404)[1]]
        dup_head = full(0x405) + [full(0x405)[0]]
        overlap = [frame(ip_packet(rb(16), foff=MF, ident=0x406), tr), frame(ip_packet(rb(16), foff=1, ident=0x406), tr)]
        odd_mf = [frame(ip_packet(rb(13), foff=MF, ident=0x407), tr), frame(ip_packet(rb(8), foff=2, ident=0x407), tr)]
        reuse = full(0x408) + full(0x408)                                                     # a key used twice
        # a gap and an overlap that cancel in the sum of the lengths: [0,16) + [8,24) + [32,40), total 40
        gap_overlap = [frame(ip_packet(rb(16), foff=MF, ident=0x40A), tr), frame(ip_packet(rb(16), foff=MF | 1, ident=0x40A), tr),
                       frame(ip_packet(rb(8), foff=4, ident=0x40A), tr)]
        add("incomplete" + sfx, list(fr) + two_lasts + dup + dup_head + overlap + odd_mf + reuse + gap_overlap + full(0x409), t)
        # the same id under another source, destination or protocol: four datagrams
        a, b, c, d = (fragments(rng, rb(70 + q), [24, 48], tr, ident=0x500, **kw)
                      for q, kw in enumerate(({}, dict(src=0x0A000009), dict(dst=0x0A000009), dict(proto=6))))
        add("same_id" + sfx, [x for quad in zip(a, b, c, d) for x in quad], t)
        # other traffic between the fragments, groups interleaved and reversed
        a = fragments(rng, rb(3000), [1000, 2000], tr, ident=0x600)
        b = fragments(rng, rb(2001), [8, 16, 24, 1000], tr, ident=0x601, hlen_head=32)
        c = fragments(rng, rb(500), [248], tr, ident=0x602)
        other = [frame(rb(28), tr, etype=0x0806), frame(b"\x00\x05\x08\x00" + rb(40), tr, etype=0x8100),
                 frame(b"\x60" + rb(45), tr, etype=0x86DD)]
        add("interleaved" + sfx, [b[4], a[0], other[0], c[1], b[0], a[2], other[1], b[2], good(8), c[0], b[3], other[2], a[1], b[1]], t)
        add("reversed" + sfx, (a + b + c)[::-1], t)
    # the largest datagram: 65515 payload bytes behind a 20-byte header, 45 fragments at mtu 1500
    big = rb(65515)
    add("total_65515", fragments(rng, big, list(range(1472, 65515, 1472)), True, ident=0x999)[::-1], 1)
    return C


def main():
    blob, recs = bytearray(), []
    for c in cases():
        kw = {k: c[k] for k in ("verdict", "drop_mask", "out_bytes") if k in c}
        st, dg = expect(c["frames"], c["flags"], **kw)
        rec = dict(tag=c["tag"], flags=c["flags"], verdict=c.get("verdict"), drop_mask=c.get("drop_mask", 0),
                   out_bytes=c.get("out_bytes"), at=len(blob), flen=[len(f) for f in c["frames"]], fstat=st,
                   dlead=[lead for lead, _b, _f in dg], dlen=[len(b) for _l, b, _f in dg],
                   fits=[int(f) for _l, _b, f in dg])
        for f in c["frames"]:
            blob += f
        rec["dat"] = len(blob)
        for _l, b, _f in dg:
            blob += b
        recs.append(rec)
    with open(os.path.join(HERE, "rxr_vectors.bin"), "wb") as f:
        f.write(blob)
    with open(os.path.join(HERE, "rxr_vectors.json"), "w") as f:
        json.dump({"arena": "rxr_vectors.bin", "cases": recs}, f, separators=(",", ":"))
        f.write("\n")
    seen = 0
    for r in recs:
        for s in r["fstat"]:
            seen |= s
    print(f"{len(recs)} cases, {sum(len(r['flen']) for r in recs)} frames, {sum(len(r['dlen']) for r in recs)} datagrams, "
          f"{len(blob)} bytes, status bits seen 0x{seen:03x}")


if __name__ == "__main__":
    main()
