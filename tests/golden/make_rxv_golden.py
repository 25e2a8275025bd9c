"""Generate the RX-validation fixtures (tests/golden/rxv_vectors.{bin,json}, rxv.pcap).

    python tests/golden/make_rxv_golden.py

Frames and their expected verdict words (include/nstack_rxv.h) from an INDEPENDENT formulation
written only for this script: RFC 1071 over big-endian 16-bit words, the pseudo headers of RFC 793
/ RFC 768, zlib.crc32 for the FCS, and the reference's receive predicates read from its source
(src/ip.c:130-151, src/tcp.c:496-510, src/udp.c:83, src/icmp.c:42, src/nstack_ip.h:212-215). It
does not use the oracle. The reference itself cannot produce these words: the build of src/ip.c was
refused, and its two checksum tests are under "#if 0"; as for the inet fixtures, no
output of the reference backs these vectors. tests/test_rxv_model.py checks the model
(tests/rxv_model.py, which takes its arithmetic from the oracle) against them, tests/test_gpu_rxv.py
the kernels. The frame builders below also serve those tests' built traffic.
"""
import json
import os
import random
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))

F_TRAILER = 1
FCS_BAD, RUNT, IPV4, IP_BAD_HDR, IP_BAD_LEN, IP_BAD_CSUM = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
FRAG, L4_CHECKED, L4_BAD_CSUM, L4_SHORT = 0x040, 0x080, 0x100, 0x200
RESIDUE = 0x2144DF1C


def be_sum(b: bytes) -> int:
    if len(b) & 1:
        b = b + b"\x00"
    return sum(struct.unpack(f">{len(b) // 2}H", b)) if b else 0


def fold(s: int) -> int:
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def csum(s: int) -> int:
    """The big-endian checksum field value for a sum taken with the field zeroed."""
    return ~fold(s) & 0xFFFF


def verifies(s: int) -> bool:
    """A sum taken over data that includes its checksum field: good when it folds to 0xffff (or
    every word is zero: nstack's 0xffff accumulator start then returns 0 as well)."""
    return s == 0 or fold(s) == 0xFFFF


# ---- builders ----
def ip_header(proto, seg_len, hlen=20, src=0x0A000001, dst=0x0A000002, foff=0, ident=0x1234, ip_len=None, rng=None):
    opts = bytes(rng.randrange(256) for _ in range(hlen - 20)) if rng else bytes(hlen - 20)
    h = bytearray(struct.pack(">BBHHHBBHII", 0x40 | (hlen // 4), 0, hlen + seg_len if ip_len is None else ip_len,
                              ident, foff, 64, proto, 0, src, dst) + opts)
    h[10:12] = struct.pack(">H", csum(be_sum(bytes(h))))
    return bytes(h)


def tcp_segment(payload: bytes, src, dst, sport=1234, dport=80):
    L = 20 + len(payload)
    s = bytearray(struct.pack(">HHIIBBHHH", sport, dport, 1, 2, 0x50, 0x18, 4096, 0, 0) + payload)
    s[16:18] = struct.pack(">H", csum(be_sum(struct.pack(">IIBBH", src, dst, 0, 6, L)) + be_sum(bytes(s))))
    return bytes(s)


def udp_segment(payload: bytes, src, dst, sport=53, dport=5353, zero_csum=False):
    L = 8 + len(payload)
    s = bytearray(struct.pack(">HHHH", sport, dport, L, 0) + payload)
    if not zero_csum:
        c = csum(be_sum(struct.pack(">IIBBH", src, dst, 0, 17, L)) + be_sum(bytes(s)))
        s[6:8] = struct.pack(">H", c or 0xFFFF)   # RFC 768: a computed zero goes out as all ones
    return bytes(s)


def icmp_message(payload: bytes):
    s = bytearray(struct.pack(">BBHHH", 8, 0, 0, 7, 1) + payload)
    s[2:4] = struct.pack(">H", csum(be_sum(bytes(s))))
    return bytes(s)


def with_fcs(body: bytes) -> bytes:
    return body + struct.pack("<I", zlib.crc32(body))


def frame(l3: bytes, ethertype=0x0800, pad_to=0, trailer=True, rng=None):
    mac = bytes(rng.randrange(256) for _ in range(12)) if rng else bytes(range(12))
    body = mac + struct.pack(">H", ethertype) + l3
    if len(body) < pad_to:
        body += bytes(pad_to - len(body))
    return with_fcs(body) if trailer else body


def l4_frame(kind, payload: bytes, hlen=20, pad_to=0, trailer=True, rng=None, **ipkw):
    src = rng.getrandbits(32) if rng else 0xC0A80001
    dst = rng.getrandbits(32) if rng else 0xC0A800C7
    if kind == "tcp":
        seg, proto = tcp_segment(payload, src, dst), 6
    elif kind == "udp":
        seg, proto = udp_segment(payload, src, dst), 17
    elif kind == "udp0":
        seg, proto = udp_segment(payload, src, dst, zero_csum=True), 17
    else:
        seg, proto = icmp_message(payload), 1
    return frame(ip_header(proto, len(seg), hlen, src, dst, rng=rng, **ipkw) + seg, pad_to=pad_to, trailer=trailer,
                 rng=rng)


# ---- the expected verdict, independently of the model and the oracle ----
def expect(fr: bytes, flags: int) -> int:
    F = len(fr)
    T = 4 if flags & F_TRAILER else 0
    v = 0
    if T and (F == 0 or zlib.crc32(fr) != RESIDUE):
        v |= FCS_BAD
    if F < 14 + T:
        return v | RUNT
    P = F - 14 - T
    if fr[12] != 0x08 or fr[13] != 0x00:
        return v
    v |= IPV4
    if P < 20:
        return v | IP_BAD_HDR
    vhl = fr[14]
    hlen = (vhl & 15) * 4
    if not (vhl & 0x40) or hlen < 20 or hlen > P:
        return v | IP_BAD_HDR
    ip_len = (fr[16] << 8) | fr[17]
    foff = (fr[20] << 8) | fr[21]
    proto = fr[23]
    v |= proto << 16
    if ip_len != P:
        v |= IP_BAD_LEN
    if not verifies(be_sum(fr[14:14 + hlen])):
        v |= IP_BAD_CSUM
    if foff & 0x3FFF:
        return v | FRAG
    if ip_len < hlen or ip_len > P:
        return v
    L = ip_len - hlen
    seg = fr[14 + hlen:14 + ip_len]
    addrs = be_sum(fr[26:34])
    if proto == 6:
        if L < 20:
            return v | L4_SHORT
        ok = verifies(addrs + 6 + L + be_sum(seg))
    elif proto == 17:
        if L < 8:
            return v | L4_SHORT
        if seg[6] == 0 and seg[7] == 0:
            return v
        ok = verifies(addrs + 17 + L + be_sum(seg))
    elif proto == 1:
        if L < 4:
            return v | L4_SHORT
        ok = verifies(be_sum(seg))
    else:
        return v
    return v | L4_CHECKED | (0 if ok else L4_BAD_CSUM)


def flip(fr: bytes, pos: int, refcs=False) -> bytes:
    b = bytearray(fr)
    b[pos] ^= 0x5A
    return with_fcs(bytes(b[:-4])) if refcs else bytes(b)


def main():
    rng = random.Random(0x52585631)
    frames = []   # (tag, bytes)

    def add(tag, fr):
        frames.append((tag, fr))

    for kind in ("tcp", "udp", "udp0", "icmp"):
        for hlen in (20, 24, 40, 60):
            for n in (0, 1, 2, 3, 17, 18, 19, 63, 64, 65, 255, 1000, 1459, 1460):
                add(f"{kind}_h{hlen}_p{n}", l4_frame(kind, rng.randbytes(n), hlen, rng=rng))
    for kind in ("tcp", "udp", "icmp"):                       # padded to the Ethernet minimum
        for n in (0, 1, 5):
            add(f"{kind}_pad60_p{n}", l4_frame(kind, rng.randbytes(n), pad_to=60, rng=rng))
    add("jumbo_tcp", l4_frame("tcp", rng.randbytes(8960), rng=rng))
    add("jumbo_udp_h60", l4_frame("udp", rng.randbytes(8901), 60, rng=rng))
    add("icmp_zeros", frame(ip_header(1, 8) + bytes(8)))      # all-zero message: ip_checksum returns 0
    add("arp", frame(rng.randbytes(28), ethertype=0x0806, pad_to=60))
    add("vlan", frame(rng.randbytes(64), ethertype=0x8100))
    add("ipv6", frame(rng.randbytes(80), ethertype=0x86DD))
    add("runt17", with_fcs(rng.randbytes(13)))
    add("runt3", rng.randbytes(3))
    add("empty", b"")
    add("frag_mf", frame(ip_header(6, 40, foff=0x2000) + rng.randbytes(40)))
    add("frag_off", frame(ip_header(17, 40, foff=0x00B9) + rng.randbytes(40)))
    add("df_only", l4_frame("tcp", rng.randbytes(30), foff=0x4000))
    add("other_proto", frame(ip_header(47, 32) + rng.randbytes(32)))
    # one frame per defect bit
    good = l4_frame("tcp", rng.randbytes(100), rng=rng)
    add("fcs_bad", flip(good, 3))
    add("ip_short_payload", frame(rng.randbytes(19)))
    add("ip_bad_version", with_fcs(good[:14] + bytes([0x05]) + good[15:-4]))
    add("ip_hlen_small", frame(bytes([0x44]) + rng.randbytes(39)))
    add("ip_hlen_past_frame", frame(bytes([0x4F]) + rng.randbytes(39)))
    add("ip_bad_len", frame(ip_header(6, 40, ip_len=61) + tcp_segment(rng.randbytes(20), 0x0A000001, 0x0A000002)))
    add("ip_len_below_hlen", frame(ip_header(6, 40, ip_len=10) + rng.randbytes(40)))
    add("ip_bad_csum", flip(good, 14 + 8, refcs=True))
    add("tcp_bad_csum", flip(good, 14 + 20 + 25, refcs=True))
    add("tcp_short", frame(ip_header(6, 19) + rng.randbytes(19)))
    add("udp_short", frame(ip_header(17, 7) + rng.randbytes(7)))
    add("icmp_short", frame(ip_header(1, 3) + rng.randbytes(3)))
    u = l4_frame("udp", rng.randbytes(77), rng=rng)
    add("udp_bad_csum", flip(u, len(u) - 5, refcs=True))
    ic = l4_frame("icmp", rng.randbytes(56), rng=rng)
    add("icmp_bad_csum", flip(ic, 14 + 20, refcs=True))
    for _ in range(60):                                         # random defects
        fr = l4_frame(rng.choice(["tcp", "udp", "icmp"]), rng.randbytes(rng.randrange(0, 600)),
                      rng.choice([20, 24, 40, 60]), rng=rng)
        add("rand_flip", flip(fr, rng.randrange(len(fr)), refcs=rng.random() < 0.5))

    arena = bytearray()
    recs = []
    for tag, fr in frames:
        arena.extend(rng.randbytes(rng.randrange(0, 16)))       # every start alignment mod 16
        recs.append({"tag": tag, "off": len(arena), "len": len(fr), "expect_trailer": expect(fr, F_TRAILER),
                     "expect_plain": expect(fr, 0)})
        arena.extend(fr)
    arena.extend(rng.randbytes(16))

    # sanity of the generator itself: the clean frames are clean, each defect frame shows its bit
    by = {r["tag"]: r for r in recs}
    assert by["tcp_h20_p1460"]["expect_trailer"] == IPV4 | L4_CHECKED | (6 << 16), hex(by["tcp_h20_p1460"]["expect_trailer"])
    assert by["udp0_h24_p17"]["expect_trailer"] == IPV4 | (17 << 16)
    assert by["icmp_zeros"]["expect_trailer"] == IPV4 | L4_CHECKED | (1 << 16)
    for tag, bit in (("fcs_bad", FCS_BAD), ("runt17", RUNT), ("ip_bad_version", IP_BAD_HDR), ("ip_bad_len", IP_BAD_LEN),
                     ("ip_bad_csum", IP_BAD_CSUM), ("frag_mf", FRAG), ("tcp_bad_csum", L4_BAD_CSUM),
                     ("udp_bad_csum", L4_BAD_CSUM), ("icmp_bad_csum", L4_BAD_CSUM), ("tcp_short", L4_SHORT),
                     ("tcp_pad60_p0", IP_BAD_LEN)):
        assert by[tag]["expect_trailer"] & bit, (tag, hex(by[tag]["expect_trailer"]))
    assert not by["tcp_bad_csum"]["expect_trailer"] & (FCS_BAD | IP_BAD_CSUM)

    with open(os.path.join(HERE, "rxv_vectors.bin"), "wb") as f:
        f.write(bytes(arena))
    # a classic little-endian pcap (link type 1) of the frames up to 1600 bytes
    small = [(r, fr) for r, (_, fr) in zip(recs, frames) if len(fr) <= 1600][::3]
    with open(os.path.join(HERE, "rxv.pcap"), "wb") as f:
        f.write(struct.pack("<IHHiIII", 0xA1B2C3D4, 2, 4, 0, 0, 65535, 1))
        for k, (_, fr) in enumerate(small):
            f.write(struct.pack("<IIII", 1700000000 + k, k, len(fr), len(fr)) + fr)
    with open(os.path.join(HERE, "rxv_vectors.json"), "w") as f:
        json.dump({"arena": "rxv_vectors.bin", "frames": recs, "pcap": "rxv.pcap",
                   "pcap_frames": [{"tag": r["tag"], "len": r["len"], "expect_trailer": r["expect_trailer"],
                                    "expect_plain": r["expect_plain"]} for r, _ in small],
                   "generator": "tests/golden/make_rxv_golden.py (independent RFC 1071 / zlib witness)"}, f, indent=0)
    print(f"{len(recs)} frames, {len(arena)} arena bytes, {len(small)} pcap frames")


if __name__ == "__main__":
    main()
