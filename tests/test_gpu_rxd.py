"""GPU tests of reassembly with L4 verdicts (include/nstack_rxd.h) through the C ABI. Every batch
asserts two things: the output arena (canaries included) and the final status words are what the
plain build's model expects (tests/rxr_model.py), and dverdict[:m] and bad equal the verdict model
(tests/rxd_model.py: the header's rules with the oracle's checksums).

What case 2 can tell apart: an unfragmented datagram whose IP header checksum byte is bent (its
header no longer sums to 0xffff) gets a wrong verdict when the header is not taken out of the sum; a
valid datagram whose fragments begin or end at odd addresses does when bytes stored to odd addresses
are not shifted; a valid datagram at an odd doff does when the parity swap is skipped."""
import struct

import numpy as np
import pytest

import nstack_amd as na
import rxd_model as rd
import rxr_model as rr
import txf_model as fm
from rxd_batch import VARIANTS, DBatch, Traffic, framed, whole_mix
from rxr_batch import mg, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
CLEAN = rd.L4_CHECKED


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def traffic(inet_oracle):
    return Traffic(inet_oracle)


# ---- 1. the rxr golden batches ----
@pytest.mark.parametrize("align", [1, 16])
def test_golden_batches(dev, inet_oracle, align):
    seen = 0
    for c in rr.load_golden()["cases"]:
        b = DBatch(inet_oracle, c["frames"], c["flags"], c["verdict"], c["drop_mask"], align, lead=align & 3, gap=1,
                   out_base=5 * align & 15, out_bytes=c["out_bytes"], seed=align)
        b.check_l4_dev(b.run_l4_dev(dev))
        for v in b.dverdict:
            seen |= int(v) & 0xFFFF
    assert seen & rd.L4_BAD_CSUM and seen & rd.NO_ROOM                   # random payloads: mostly bad, and that is fine
    assert na.rxd_last_launch() == "general-l4"


# ---- 2. valid and corrupted traffic ----
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_valid_traffic_at_every_alignment(dev, inet_oracle, traffic, lead):
    starts = set()
    for out_base in range(4):
        b = DBatch(inet_oracle, traffic.frames, rr.F_TRAILER, align=1, lead=lead, out_base=out_base, seed=out_base)
        assert b.m == len(traffic.groups) and (b.dverdict & 0xFFFF == CLEAN).all() and b.bad == 0
        r = b.run_l4_dev(dev)
        b.check_l4_dev(r)
        rest = [i for g in traffic.groups for i in g[1:]]
        starts |= {(out_base + int(b.plan["dst"][i])) & 15 for i in rest}
        assert {int(d) & 1 for d in b.plan["doff"][:b.m]} == {0, 1}
        assert {(b.plan["cls"][g[0]][1]) for g in traffic.groups} == {20, 24, 60}
    assert starts == set(range(16))


@pytest.mark.parametrize("which", VARIANTS)
def test_one_bit_variants_turn_exactly_their_datagram_bad(dev, inet_oracle, traffic, which):
    m = len(traffic.groups)
    base = DBatch(inet_oracle, traffic.frames, rr.F_TRAILER, align=1).dverdict
    for q, sel in enumerate((range(0, m, 2), range(1, m, 2))):
        frames, hit = traffic.bent(which, sel)
        b = DBatch(inet_oracle, frames, rr.F_TRAILER, align=1, lead=q + 1, out_base=2 * q + 1, seed=q)
        want = base.copy()
        want[hit] |= rd.L4_BAD_CSUM
        assert np.array_equal(b.dverdict, want) and b.bad == len(hit)    # the model: exactly these
        assert bool(hit) == (which in ("front", "line", "tail", "src", "dst"))
        b.check_l4_dev(b.run_l4_dev(dev))


# ---- 3. the short and unchecked rules ----
def test_short_segments_unchecked_udp_and_other_protocols(dev, inet_oracle):
    rng = mg.random.Random(5)
    rb = lambda n: bytes(rng.randrange(256) for _ in range(n))
    cases = [(6, 19, rd.L4_SHORT), (6, 20, CLEAN), (17, 7, rd.L4_SHORT), (17, 8, CLEAN), (1, 3, rd.L4_SHORT), (1, 4, CLEAN),
             (47, 40, 0), (17, 0, rd.L4_SHORT), (47, 0, 0)]
    frames, want = [], []
    for q, (proto, L, bits) in enumerate(cases):
        seg = bytearray(rb(L))
        if proto == 17 and L >= 8:
            seg[6:8] = b"\x12\x34"
        for hl in (20, 60):
            frames.append(mg.frame(mg.ip_packet(bytes(seg), hl, ident=q, proto=proto, rng=rng), False))
            want.append((proto << 16) | bits)
        if L >= 16:                                                      # the same datagram in two fragments
            frames += mg.fragments(rng, bytes(seg), [8], False, hlen_head=24, ident=0x100 + q, proto=proto)
            want.append((proto << 16) | bits)
    udp0 = bytearray(rd.segment(inet_oracle, "udp", rb(33), 3, 4))
    udp0[6:8] = b"\x00\x00"                                              # "no checksum": not checked, not bad
    frames += mg.fragments(rng, bytes(udp0), [16], False, ident=0x200, src=3, dst=4)
    want.append(17 << 16)
    b = DBatch(inet_oracle, frames, 0, align=1, lead=1, out_base=3)
    assert (b.dverdict & ~np.uint32(rd.L4_BAD_CSUM)).tolist() == want
    b.check_l4_dev(b.run_l4_dev(dev))


# ---- 4. the bounds of the accumulator ----
@pytest.mark.parametrize("tag,mtu,cnt", [("max_m76_h60", 76, 8185), ("max_m1500_h20", 1500, 45)])
def test_the_largest_datagrams_all_ones(dev, inet_oracle, tag, mtu, cnt):
    """65535 bytes of TCP whose payload is 0xff throughout: every frame adds the largest part there is."""
    g = fm.load_golden()
    r = next(r for r in g["datagrams"] if r["tag"] == tag)
    hdr = bytearray(g["input_bytes"][r["off"]:r["off"] + r["len"]][:(g["input_bytes"][r["off"]] & 15) * 4])
    hdr[9] = 6
    src, dst = struct.unpack_from(">II", hdr, 12)
    dg = bytes(hdr) + rd.tcp_segment(inet_oracle, b"\xff" * (65535 - len(hdr) - 20), src, dst)
    d_out, slot, first, flen = framed(dev, [dg], mtu, np.zeros((1, 12), dtype=np.uint8))
    assert int(first[1]) == cnt and len(dg) == 65535
    perm = np.random.default_rng(cnt).permutation(cnt)
    arena = d_out.cpu().numpy()
    for flip in (False, True):
        a = arena.copy()
        if flip:                                                         # one bit of the last fragment's last payload byte
            at = (cnt - 1) * slot
            a[at + 14 + ((int(a[at + 16]) << 8) | int(a[at + 17])) - 1] ^= 0x01
        b = DBatch(inet_oracle, flags=rr.F_TRAILER, align=16, placed=(a, perm.astype(np.uint64) * slot, flen[perm] + 4))
        assert b.m == 1 and int(b.plan["dlen"][0]) == 65535
        assert int(b.dverdict[0]) == (6 << 16) | CLEAN | (rd.L4_BAD_CSUM if flip else 0)
        b.check_l4_dev(b.run_l4_dev(dev))


# ---- 5. agreement with the validator ----
def test_unfragmented_frames_get_the_validators_l4_bits(dev, inet_oracle):
    frames = whole_mix(inet_oracle)
    b = DBatch(inet_oracle, frames, rr.F_TRAILER, align=1, lead=3, out_base=1)
    assert b.m == len(frames)
    r = b.run_l4_dev(dev)
    b.check_l4_dev(r)
    d_arena, d_off, d_ln = to_dev(b.arena, dev), to_dev(b.off, dev), to_dev(b.ln, dev)
    d_v = torch.zeros(b.n, dtype=torch.int32, device=dev)
    na.rx_validate_dev(d_arena, b.arena.size, d_off, d_ln, d_v, b.n, flags=na.RXV_F_TRAILER)
    torch.cuda.synchronize()
    rxv = d_v.cpu().numpy().view(np.uint32)
    assert np.array_equal(r["dverdict"][:b.m] & rd.L4_BITS, rxv & rd.L4_BITS)
    assert (rxv & na.RXV_L4_BAD_CSUM).any() and (rxv & na.RXV_L4_SHORT).any() and (rxv & na.RXV_L4_CHECKED).any()


# ---- 6. scale and determinism ----
def scale_batch(inet_oracle, n, seed):
    """n frames from a small pool of valid and bent datagrams, whole and fragmented, restamped with
    sequential ids (the id is no part of an L4 sum), shuffled within windows of 48 frames."""
    rng = mg.random.Random(seed)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    pool = []
    for q, (kind, k, cuts, hh) in enumerate((("udp", 0, None, 20), ("tcp", 33, None, 24), ("icmp", 100, None, 60), ("udp", 9, [8], 20),
                                             ("tcp", 41, [16], 24), ("icmp", 101, [32, 64], 60), ("udp", 31, [8, 16, 24], 20),
                                             ("tcp", 77, [40], 20))):
        seg = rd.segment(inet_oracle, kind, rb(k), 0x0A000001 + q, 0x0A000002)
        if q in (1, 5):
            seg = seg[:-1] + bytes([seg[-1] ^ 1])
        kw = dict(src=0x0A000001 + q, dst=0x0A000002, proto=rd.PROTO[kind])
        pool.append([mg.frame(mg.ip_packet(seg, hh, rng=rng, **kw), True)] if cuts is None else
                    mg.fragments(rng, seg, cuts, True, hlen_head=hh, hlen_rest=20, **kw))
    pool.append(mg.fragments(rng, rb(64), [32], True, proto=60)[:1])    # a lone fragment
    frames, q = [], 0
    while len(frames) < n:
        t = pool[(q * 7 + q // 11) % len(pool)]
        ident = struct.pack(">H", q & 0xFFFF)
        frames += [f[:18] + ident + f[20:] for f in t]
        q += 1
    frames = frames[:n]
    order = np.arange(n)
    prng = np.random.default_rng(seed)
    for s in range(0, n, 48):
        order[s:s + 48] = prng.permutation(order[s:s + 48])
    return DBatch(inet_oracle, [frames[i] for i in order], rr.F_TRAILER, align=1, lead=1, seed=seed)


@pytest.mark.parametrize("n", [257, 65537])
def test_scale_and_determinism(dev, inet_oracle, n):
    b = scale_batch(inet_oracle, n, n & 0xFFFF)
    assert b.m > n // 8 and 0 < b.bad < b.m // 2 and (b.fstat & rr.INCOMPLETE).any()
    runs = [b.run_l4_dev(dev) for _ in range(3)]
    for r in runs:
        b.check_l4_dev(r)
    for r in runs[1:]:
        assert np.array_equal(r["dverdict"], runs[0]["dverdict"]) and r["bad"] == runs[0]["bad"]
        assert np.array_equal(r["out"], runs[0]["out"]) and np.array_equal(r["final"], runs[0]["final"])


# ---- 7. room ----
def small_batch(inet_oracle, **kw):
    rng = mg.random.Random(7)
    rb = lambda k: bytes(rng.randrange(256) for _ in range(k))
    seg = [rd.segment(inet_oracle, "udp", rb(n), 1, 2) for n in (32, 92, 0)]
    kwp = dict(src=1, dst=2)
    frames = [mg.frame(mg.ip_packet(seg[0], ident=1, **kwp), False)] + mg.fragments(rng, seg[1], [48], False, ident=2, **kwp)[::-1] + \
             [mg.frame(mg.ip_packet(seg[2][:7], 24, ident=3, rng=rng, **kwp), False)]
    return DBatch(inet_oracle, frames, 0, bad_mask=rd.NO_ROOM | rd.L4_SHORT, **kw)


def test_room_exact_and_short(dev, inet_oracle):
    full = small_batch(inet_oracle)
    assert full.m == 3 and full.need == 60 + 120 + 31
    assert full.dverdict.tolist() == [(17 << 16) | CLEAN, (17 << 16) | CLEAN, (17 << 16) | rd.L4_SHORT] and full.bad == 1
    for out_bytes, fits in ((full.need, 3), (full.need - 1, 2), (60 + 119, 1), (59, 0), (0, 0)):
        b = small_batch(inet_oracle, out_bytes=out_bytes, out_base=3)
        assert b.dverdict[:fits].tolist() == full.dverdict[:fits].tolist()          # the others keep their verdicts
        assert (b.dverdict[fits:] == rd.NO_ROOM).all() and b.bad == 3 - fits + (fits == 3)
        b.check_l4_dev(b.run_l4_dev(dev))                               # the canaries around `out` included


def test_no_frames_and_no_bad_pointer(dev, inet_oracle):
    b = DBatch(inet_oracle, [], 0)
    r = b.run_l4_dev(dev)
    assert r["counts"].tolist() == [0, 0] and np.array_equal(r["out"], b.expect) and r["bad"] == 0
    assert (r["dverdict"] == 0x55555555).all()
    assert na.rx_reasm_l4_host(b.arena, 0, b.off, b.ln, 0, b.out0, 0, None) == (0, 0)
    b = small_batch(inet_oracle, align=16)
    b.check_l4_dev(b.run_l4_dev(dev, bad=False), bad=False)


# ---- 8. the host form ----
def test_host_form_on_the_valid_and_corrupted_traffic(dev, inet_oracle, traffic):
    m = len(traffic.groups)
    b = DBatch(inet_oracle, traffic.frames, rr.F_TRAILER, align=1, lead=1)
    assert np.array_equal(b.check_l4_host(), b.run_l4_dev(dev)["dverdict"][:m])
    for q, which in enumerate(VARIANTS):
        frames, hit = traffic.bent(which, range(q & 1, m, 2))
        b = DBatch(inet_oracle, frames, rr.F_TRAILER, align=1, lead=q & 3)
        assert b.bad == len(hit)
        b.check_l4_host()


def test_host_form_across_a_chunk_cut(dev, inet_oracle):
    """65537 whole 60-byte datagrams: kChunkDgs cuts them into two chunks; the verdicts cross the cut."""
    rng = mg.random.Random(9)
    pool = []
    for q in range(5):
        seg = rd.segment(inet_oracle, "udp", bytes(rng.randrange(256) for _ in range(32)), 0x0A000001 + q, 0x0A000002)
        if q == 3:
            seg = seg[:20] + bytes([seg[20] ^ 0x40]) + seg[21:]
        pool.append(mg.frame(mg.ip_packet(seg, ident=0, src=0x0A000001 + q, dst=0x0A000002), False))
    n = 65537
    frames = [pool[(q * 3 + q // 7) % 5] for q in range(n)]
    b = DBatch(inet_oracle, frames, 0, align=1)
    assert b.m == n and (b.plan["dlen"] == 60).all()
    dv = b.check_l4_host(cut=[65536, 1])
    assert dv[65535] == b.dverdict[65535] and dv[65536] == b.dverdict[65536] and 0 < b.bad < n


# ---- 9. launch names ----
def test_launch_names(dev, inet_oracle):
    b = small_batch(inet_oracle)
    b.check_l4_dev(b.run_l4_dev(dev))
    assert na.rxd_last_launch() == "general-l4"
    b.check_dev(b.run_dev(dev))
    assert na.rxr_last_launch() == "general" and na.rxd_last_launch() == "general-l4"
