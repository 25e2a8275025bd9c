"""Generate the TX-sealing fixtures (tests/golden/txs_vectors.json, txs_input.bin, txs_sealed_f{0..3}.bin).

    python tests/golden/make_txs_golden.py

Unsealed frames (every checksum field filled with garbage, four garbage bytes behind each frame) and
what sealing must make of them (include/nstack_txs.h) under each of the four flag combinations,
from an INDEPENDENT formulation written only for this script and make_rxv_golden.py, whose frame
builders it uses: RFC 1071 over big-endian 16-bit words, the pseudo headers of RFC 793 / RFC 768,
zlib.crc32 for the FCS. It does not use the oracle or the model. The one place where the reference
departs from RFC 1071 is restated by hand: ip_checksum and tcp_checksum start their accumulator at
0xffff (src/ip.c:42, src/tcp.c:172), so data whose words are all zero gives 0, not 0xffff.
tests/test_txs_model.py checks the model (tests/txs_model.py, which takes its arithmetic from the
oracle) against these vectors, tests/test_gpu_txs.py the kernels.
"""
import importlib.util
import json
import os
import random
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_rxv_golden", os.path.join(HERE, "make_rxv_golden.py"))
rx = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(rx)

F_FCS, F_UDP_ZERO = 1, 2
FCS_SET, RUNT, IPV4, IP_BAD_HDR, IP_BAD_LEN, IP_CSUM_SET = 0x001, 0x002, 0x004, 0x008, 0x010, 0x020
FRAG, L4_CSUM_SET, L4_SHORT = 0x040, 0x080, 0x200
ALL_BITS = (FCS_SET, RUNT, IPV4, IP_BAD_HDR, IP_BAD_LEN, IP_CSUM_SET, FRAG, L4_CSUM_SET, L4_SHORT)


def ref_csum(s: int) -> int:
    """The big-endian field value of the reference's 0xffff-start functions for a sum taken with the
    field zeroed: RFC 1071's, but 0 when every word is zero."""
    return 0 if s == 0 else rx.csum(s)


def native(be_value: int) -> int:
    """The uint16_t a little-endian host reads from the two bytes a big-endian value is stored as."""
    return ((be_value & 0xFF) << 8) | (be_value >> 8)


def expect(fr: bytes, flags: int):
    """(sealed bytes: F, plus 4 with F_FCS; status; [ip_csum, l4_csum, fcs]; positions of the
    checksum fields sealing writes)."""
    b = bytearray(fr)
    F = len(b)
    st, ip, l4, fcs, pos = 0, 0, 0, 0, []

    def l3l4():
        nonlocal st, ip, l4
        if F < 14:
            st |= RUNT
            return
        if b[12] != 0x08 or b[13] != 0x00:
            return
        st |= IPV4
        P = F - 14
        if P < 20:
            st |= IP_BAD_HDR
            return
        vhl = b[14]
        hlen = (vhl & 15) * 4
        if not (vhl & 0x40) or hlen < 20 or hlen > P:
            st |= IP_BAD_HDR
            return
        proto = b[23]
        st |= (proto << 16) | IP_CSUM_SET
        b[24:26] = b"\x00\x00"
        c = ref_csum(rx.be_sum(bytes(b[14:14 + hlen])))
        b[24:26] = struct.pack(">H", c)
        ip = native(c)
        pos.append(24)
        ip_len = (b[16] << 8) | b[17]
        foff = (b[20] << 8) | b[21]
        bad_len = ip_len < hlen or ip_len > P
        if bad_len:
            st |= IP_BAD_LEN
        if foff & 0x3FFF:
            st |= FRAG
        if bad_len or foff & 0x3FFF:
            return
        L = ip_len - hlen
        s0 = 14 + hlen
        if proto not in (6, 17, 1):
            return
        if L < {6: 20, 17: 8, 1: 4}[proto]:
            st |= L4_SHORT
            return
        q = s0 + {6: 16, 17: 6, 1: 2}[proto]
        pos.append(q)
        b[q:q + 2] = b"\x00\x00"
        seg = bytes(b[s0:s0 + L])
        addrs = rx.be_sum(bytes(b[26:34]))
        if proto == 6:
            c = ref_csum(addrs + 6 + L + rx.be_sum(seg))
        elif proto == 17:
            if flags & F_UDP_ZERO:
                return
            c = rx.csum(addrs + 17 + L + rx.be_sum(seg)) or 0xFFFF
        else:
            c = ref_csum(rx.be_sum(seg))
        b[q:q + 2] = struct.pack(">H", c)
        l4 = native(c)
        st |= L4_CSUM_SET

    l3l4()
    if flags & F_FCS:
        fcs = zlib.crc32(bytes(b))
        b += struct.pack("<I", fcs)
        st |= FCS_SET
    return bytes(b), st, [ip, l4, fcs], pos


def garble(fr: bytes, rng) -> bytes:
    """The frame with garbage in every checksum field sealing would write."""
    b = bytearray(fr)
    for q in expect(fr, 0)[3]:
        b[q:q + 2] = rng.randbytes(2)
    return bytes(b)


def udp_summing_to_zero(rng, hlen=20, n=40):
    """A UDP frame whose checksum computes to 0 (and goes out as 0xffff): the payload's last word
    makes the pseudo header and segment sum to 0xffff."""
    src, dst = 0xC0A80001, 0xC0A800C7
    L = 8 + n
    pay = bytearray(rng.randbytes(n - 2) + b"\x00\x00")
    seg = struct.pack(">HHHH", 53, 5353, L, 0) + bytes(pay)
    s0 = rx.fold(rx.be_sum(struct.pack(">IIBBH", src, dst, 0, 17, L)) + rx.be_sum(seg))
    pay[-2:] = struct.pack(">H", 0xFFFF - s0)
    seg = struct.pack(">HHHH", 53, 5353, L, 0) + bytes(pay)
    assert rx.csum(rx.be_sum(struct.pack(">IIBBH", src, dst, 0, 17, L)) + rx.be_sum(seg)) == 0
    return rx.frame(rx.ip_header(17, L, hlen, src, dst) + seg, trailer=False)


def build_frames(rng):
    """[(tag, unsealed frame)]; every checksum field garbage."""
    frames = []

    def add(tag, fr):
        frames.append((tag, garble(fr, rng)))

    for kind in ("tcp", "udp", "icmp"):
        for hlen in range(20, 64, 4):                               # all eleven header lengths
            for n in (0, 1, 2, 3, 17, 64, 255, 1000, 1459):
                add(f"{kind}_h{hlen}_p{n}", rx.l4_frame(kind, rng.randbytes(n), hlen, trailer=False, rng=rng))
    for kind in ("tcp", "udp", "icmp"):                             # padded to the Ethernet minimum
        for n in (0, 1, 5):
            add(f"{kind}_pad60_p{n}", rx.l4_frame(kind, rng.randbytes(n), pad_to=60, trailer=False, rng=rng))
    add("tcp_trailing_junk", rx.l4_frame("tcp", rng.randbytes(33), 24, trailer=False, rng=rng) + rng.randbytes(7))
    add("jumbo_tcp", rx.l4_frame("tcp", rng.randbytes(8964), trailer=False, rng=rng))
    add("jumbo_udp_h60", rx.l4_frame("udp", rng.randbytes(8901), 60, trailer=False, rng=rng))
    add("jumbo_icmp_h44", rx.l4_frame("icmp", rng.randbytes(4001), 44, trailer=False, rng=rng))
    add("udp_sums_to_zero", udp_summing_to_zero(rng))
    add("udp_sums_to_zero_h36", udp_summing_to_zero(rng, 36, 300))
    add("icmp_zeros", rx.frame(rx.ip_header(1, 8) + bytes(8), trailer=False))   # ip_checksum of zeros is 0
    add("arp", rx.frame(rng.randbytes(28), ethertype=0x0806, pad_to=60, trailer=False))
    add("vlan", rx.frame(rng.randbytes(64), ethertype=0x8100, trailer=False))
    add("ipv6", rx.frame(rng.randbytes(80), ethertype=0x86DD, trailer=False))
    add("runt13", rng.randbytes(13))
    add("runt3", rng.randbytes(3))
    add("empty", b"")
    add("eth_only", rx.frame(b"", trailer=False))
    add("frag_mf", rx.frame(rx.ip_header(6, 40, foff=0x2000) + rng.randbytes(40), trailer=False))
    add("frag_off", rx.frame(rx.ip_header(17, 40, foff=0x00B9) + rng.randbytes(40), trailer=False))
    add("frag_and_bad_len", rx.frame(rx.ip_header(17, 40, foff=0x2001, ip_len=900) + rng.randbytes(40), trailer=False))
    add("df_only", rx.l4_frame("tcp", rng.randbytes(30), foff=0x4000, trailer=False))
    add("other_proto", rx.frame(rx.ip_header(47, 32) + rng.randbytes(32), trailer=False))
    good = rx.l4_frame("tcp", rng.randbytes(100), trailer=False, rng=rng)
    add("ip_short_payload", rx.frame(rng.randbytes(19), trailer=False))
    add("ip_bad_version", good[:14] + bytes([0x05]) + good[15:])
    add("ip_hlen_small", rx.frame(bytes([0x44]) + rng.randbytes(39), trailer=False))
    add("ip_hlen_past_frame", rx.frame(bytes([0x4F]) + rng.randbytes(39), trailer=False))
    add("ip_len_past_frame", rx.frame(rx.ip_header(6, 40, ip_len=61) + rng.randbytes(40), trailer=False))
    add("ip_len_below_hlen", rx.frame(rx.ip_header(6, 40, ip_len=10) + rng.randbytes(40), trailer=False))
    add("tcp_short", rx.frame(rx.ip_header(6, 19) + rng.randbytes(19), trailer=False))
    add("udp_short", rx.frame(rx.ip_header(17, 7) + rng.randbytes(7), trailer=False))
    add("icmp_short", rx.frame(rx.ip_header(1, 3) + rng.randbytes(3), trailer=False))
    add("tcp_min", rx.frame(rx.ip_header(6, 20) + rng.randbytes(20), trailer=False))
    add("udp_min", rx.frame(rx.ip_header(17, 8) + rng.randbytes(8), trailer=False))
    add("icmp_min_h60", rx.frame(rx.ip_header(1, 4, 60, rng=rng) + rng.randbytes(4), trailer=False))
    return frames


def main():
    rng = random.Random(0x54585331)
    frames = build_frames(rng)
    arena = bytearray()
    recs = []
    for tag, fr in frames:
        arena.extend(rng.randbytes(rng.randrange(0, 16)))          # every start alignment mod 16
        recs.append({"tag": tag, "off": len(arena), "len": len(fr), "status": [], "fields": []})
        arena.extend(fr)
        arena.extend(rng.randbytes(4))                              # the FCS place: garbage
    arena.extend(rng.randbytes(16))
    sealed = [bytearray(arena) for _ in range(4)]
    for flags in range(4):
        for r, (_, fr) in zip(recs, frames):
            out, st, fl, _ = expect(fr, flags)
            sealed[flags][r["off"]:r["off"] + len(out)] = out
            r["status"].append(st)
            r["fields"].append(fl)

    # sanity of the generator itself
    by = {r["tag"]: r for r in recs}
    seen = 0
    for r in recs:
        seen |= r["status"][F_FCS]
    for bit in ALL_BITS:
        assert seen & bit, hex(bit)
    assert by["tcp_h20_p1459"]["status"][1] == FCS_SET | IPV4 | IP_CSUM_SET | L4_CSUM_SET | (6 << 16)
    assert by["udp_sums_to_zero"]["fields"][0][1] == 0xFFFF and by["udp_sums_to_zero"]["status"][0] & L4_CSUM_SET
    assert by["udp_sums_to_zero"]["fields"][2][1] == 0 and not by["udp_sums_to_zero"]["status"][2] & L4_CSUM_SET
    assert by["icmp_zeros"]["fields"][0][1] == 0 and by["icmp_zeros"]["status"][0] & L4_CSUM_SET
    assert by["frag_and_bad_len"]["status"][0] & (FRAG | IP_BAD_LEN) == FRAG | IP_BAD_LEN
    for r, (_, fr) in zip(recs, frames):                            # a sealed frame passes the receive checks
        v = rx.expect(bytes(sealed[1][r["off"]:r["off"] + r["len"] + 4]), rx.F_TRAILER)
        assert not v & (rx.FCS_BAD | rx.IP_BAD_CSUM | rx.L4_BAD_CSUM), (r["tag"], hex(v))
        if r["status"][1] & L4_CSUM_SET:
            assert v & rx.L4_CHECKED, r["tag"]
    for flags in range(4):                                          # nothing but fields and FCS places differs
        diff = sum(1 for a, b in zip(arena, sealed[flags]) if a != b)
        assert diff <= sum(2 * len(expect(fr, flags)[3]) + (4 if flags & F_FCS else 0) for _, fr in frames)

    with open(os.path.join(HERE, "txs_input.bin"), "wb") as f:
        f.write(bytes(arena))
    for flags in range(4):
        with open(os.path.join(HERE, f"txs_sealed_f{flags}.bin"), "wb") as f:
            f.write(bytes(sealed[flags]))
    with open(os.path.join(HERE, "txs_vectors.json"), "w") as f:
        json.dump({"input": "txs_input.bin", "sealed": [f"txs_sealed_f{k}.bin" for k in range(4)], "frames": recs,
                   "generator": "tests/golden/make_txs_golden.py (independent RFC 1071 / zlib witness); status and "
                                "fields are indexed by the flags value 0..3"}, f, indent=0)
    print(f"{len(recs)} frames, {len(arena)} arena bytes")


if __name__ == "__main__":
    main()
