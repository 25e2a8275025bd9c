"""GPU tests of one-pass RX coalescing (include/nstack_gro.h) through the C ABI. Every batch asserts
that the plan arrays, the whole output arena (canary bytes in front of, between and behind the
datagrams included), the final status words, the datagram verdict words and `bad` are exactly what
the model expects (tests/gro_model.py: the header's rules with the oracle's checksums). Whole-arena
equality is also what shows a write outside a datagram's own range."""
import struct

import numpy as np
import pytest

import gro_model as gm
import nstack_amd as na
import rxd_model as rd
import rxr_model as rr
import tso_model as tm
import txf_model as fm
from gro_batch import ALL_FLAGS, GBatch, cut, mixed_no_group, payload, stays_apart, tso_datagrams
from rxr_batch import host_chunks, mg, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
MERGED_WORD = gm.GROD_MERGED | (6 << rd.PROTO_SHIFT)
TCP_OK = (6 << rd.PROTO_SHIFT) | rd.L4_CHECKED
MAC = bytes(range(0x20, 0x2C))
MTU = 1500
DROP = na.RXV_FCS_BAD | na.RXV_IP_BAD_HDR | na.RXV_IP_BAD_CSUM | na.RXV_L4_BAD_CSUM


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def assert_checksums(inet_oracle, b, out):
    """Test 6: every delivered merged datagram of the device's arena has tcp_checksum == 0 and a header
    ip_checksum == 0, by the oracle's own functions."""
    seen = 0
    for k, dg in enumerate(b.datagrams(out)):
        if int(b.dverdict[k]) != MERGED_WORD:
            continue
        hlen = (dg[0] & 15) * 4
        src, dst = struct.unpack_from(">II", dg, 12)
        assert inet_oracle.oracle_ip_checksum(dg[:hlen], hlen) == 0, k
        assert inet_oracle.oracle_tcp_checksum(src, dst, dg[hlen:], len(dg) - hlen) == 0, k
        assert struct.unpack_from(">H", dg, 2)[0] == len(dg)
        seen += 1
    return seen


# ---- 1. the inverse of segmentation ----
def tso_dev(dev, dgs, mss, id_fixed):
    """ip_tx_tso_dev at mtu 1500 with the FCS over the datagrams: (arena, slot, flen without the FCS)."""
    flags = fm.F_FCS | fm.F_L2_ONE | tm.F_MSS_ONE | (tm.F_ID_FIXED if id_fixed else 0)
    arena = np.frombuffer(b"".join(dgs), dtype=np.uint8)
    ln = np.array([len(d) for d in dgs], dtype=np.uint32)
    off = np.zeros(len(dgs), dtype=np.uint64)
    off[1:] = np.cumsum(ln[:-1], dtype=np.uint64)
    n, slot = len(dgs), fm.min_slot(MTU, fm.F_FCS)
    d_arena, d_off, d_ln = (to_dev(x, dev) for x in (arena, off, ln))
    d_l2 = to_dev(np.frombuffer(MAC, dtype=np.uint8).reshape(1, 12), dev)
    d_mss = to_dev(np.array([mss], dtype=np.uint16).view(np.int16), dev)
    d_first = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    na.tx_tso_plan_dev(d_arena, arena.size, d_off, d_ln, d_mss, n, MTU, d_first, flags)
    torch.cuda.synchronize()
    slots = int(d_first.cpu().numpy().view(np.uint64)[n])
    d_out = torch.full((slots * slot + 16,), 0xEE, dtype=torch.uint8, device=dev)
    d_flen = torch.zeros(slots, dtype=torch.int32, device=dev)
    na.tx_tso_dev(d_arena, arena.size, d_off, d_ln, d_l2, d_mss, n, MTU, d_first, d_out, slot, slots, flags, d_flen)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), slot, d_flen.cpu().numpy().view(np.uint32)


def validated(dev, arena, off, ln):
    d_v = torch.zeros(len(off), dtype=torch.int32, device=dev)
    na.rx_validate_dev(to_dev(arena, dev), arena.size, to_dev(off, dev), to_dev(ln, dev), d_v, len(off), na.RXV_F_TRAILER)
    torch.cuda.synchronize()
    return d_v.cpu().numpy().view(np.uint32)


def segmented_batch(dev, inet_oracle, mss, id_fixed, **kw):
    """(batch, datagrams, frames as bytes in slot order): cut by ip_tx_tso_dev, judged by
    ether_rx_validate_dev, the slots named in a permuted order."""
    dgs = tso_datagrams(inet_oracle, mss)
    arena, slot, flen = tso_dev(dev, dgs, mss, id_fixed)
    perm = np.random.default_rng(mss + id_fixed).permutation(len(flen))
    off, ln = perm.astype(np.uint64) * np.uint64(slot), (flen[perm] + 4).astype(np.uint32)
    v = validated(dev, arena, off, ln)
    assert (v & DROP == 0).all() and (v & na.RXV_L4_CHECKED != 0).all()
    b = GBatch(inet_oracle, flags=rr.F_TRAILER, verdict=v, drop_mask=DROP, placed=(arena, off, ln), **kw)
    frames = [arena[k * slot:k * slot + int(flen[k]) + 4].tobytes() for k in range(len(flen))]
    return b, dgs, frames


@pytest.mark.parametrize("id_fixed", [False, True])
@pytest.mark.parametrize("mss", [1460, 1459, 536, 7, 1])
def test_inverse_of_segmentation(dev, inet_oracle, mss, id_fixed):
    b, dgs, frames = segmented_batch(dev, inet_oracle, mss, id_fixed, align=16, out_base=mss & 3)
    assert b.m == len(dgs) and sorted(b.datagrams()) == sorted(dgs)      # the model: every datagram byte for byte
    assert (b.dverdict == MERGED_WORD).sum() >= 4 and (b.dverdict == TCP_OK).sum() >= 1
    r = b.run_gro_dev(dev)
    b.check_gro_dev(r)
    got = b.datagrams(r["out"])
    assert sorted(got) == sorted(dgs) and all(d[(d[0] & 15) * 4 + 13] == ALL_FLAGS for d in got)
    assert assert_checksums(inet_oracle, b, r["out"]) >= 4
    # and ip_tx_tso_dev over the output gives the original frames back
    arena2, slot, flen2 = tso_dev(dev, got, mss, id_fixed)
    again = [arena2[k * slot:k * slot + int(flen2[k]) + 4].tobytes() for k in range(len(flen2))]
    assert sorted(again) == sorted(frames)


# ---- 2. alignment ----
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_every_alignment_of_frames_and_out(dev, inet_oracle, lead):
    """Last segments of 1..8 bytes behind odd units, so that payloads start on odd destination bytes and
    at every offset of the 16-byte grid."""
    rng = np.random.default_rng(lead)
    frames = []
    for tail in range(1, 9):
        hlen, thl = (20, 24)[tail & 1], (20, 32, 60)[tail % 3]
        dg = gm.tcp_datagram(inet_oracle, payload(rng, 3 * (31 + 2 * tail) + tail), 1000 * tail, hlen, thl, ALL_FLAGS,
                             sport=0x8000 + tail)
        frames += cut(inet_oracle, dg, 31 + 2 * tail, pad=0)[::-1]
    starts = set()
    for out_base in range(4):
        for align in (1, 16, 128):
            b = GBatch(inet_oracle, frames, 0, align=align, lead=lead, gap=1, out_base=out_base, seed=align)
            assert b.m == 8 and (b.dverdict == MERGED_WORD).all()
            r = b.run_gro_dev(dev)
            b.check_gro_dev(r)
            assert assert_checksums(inet_oracle, b, r["out"]) == 8
            starts |= {(b.base + int(d)) & 15 for i, d in enumerate(b.plan["dst"]) if not b.fstat[i] & rr.HEAD}
            assert {(b.base + int(d)) & 1 for i, d in enumerate(b.plan["dst"]) if not b.fstat[i] & rr.HEAD} == {0, 1}
    assert starts == set(range(16))
    assert {int(o) & 3 for o in b.off} == {0, 1, 2, 3}


# ---- 3. windows ----
def test_windows_wrap_and_the_size_limit(dev, inet_oracle):
    rng = np.random.default_rng(5)
    a = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 1000), (3 << 15) - 450, tflags=gm.ACK | gm.PSH), 100)
    w = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 300), (1 << 32) - 130, hlen=24, thl=32, sport=0x8100), 60)
    b = GBatch(inet_oracle, a + w[::-1], align=16, out_base=1)
    assert b.m == 4 and b.plan["dlen"].tolist() == [540, 540, 56 + 120, 56 + 180]
    assert (b.dverdict == MERGED_WORD).all()
    assert b.fstat[4] & gm.MERGED and not b.fstat[4] & rr.HEAD          # the straddling segment goes by its seq
    r = b.run_gro_dev(dev)
    b.check_gro_dev(r)
    assert assert_checksums(inet_oracle, b, r["out"]) == 4
    for I, merges in ((32768, True), (32769, False)):
        big = gm.tcp_datagram(inet_oracle, payload(rng, I - 40), 0)
        nxt = gm.tcp_datagram(inet_oracle, payload(rng, 10), I - 40)
        b = GBatch(inet_oracle, [mg.frame(nxt, False), mg.frame(big, False)], lead=1)
        assert bool(b.fstat[1] & gm.CAND) == merges and b.m == (1 if merges else 2)
        assert b.dverdict.tolist() == ([MERGED_WORD] if merges else [TCP_OK, TCP_OK])
        b.check_gro_dev(b.run_gro_dev(dev))
    # the largest merged datagram: 65535 bytes
    parts = [gm.tcp_datagram(inet_oracle, payload(rng, P), s) for s, P in ((0, 16000), (16000, 16767), (32767, 32728))]
    b = GBatch(inet_oracle, [mg.frame(p, False) for p in parts[::-1]], out_base=3)
    assert b.m == 1 and int(b.plan["dlen"][0]) == 65535
    r = b.run_gro_dev(dev)
    b.check_gro_dev(r)
    assert assert_checksums(inet_oracle, b, r["out"]) == 1


# ---- 4. what stays apart ----
def test_stays_apart(dev, inet_oracle):
    frames, verdict, mask, cases = stays_apart(inet_oracle)
    b = GBatch(inet_oracle, frames, 0, verdict, mask, lead=1, gap=1, out_base=1)
    assert not (b.fstat & gm.MERGED).any() and b.m == len(frames) - 1
    assert (b.dverdict == TCP_OK).all()                                  # each one alone, with its own nstack_rxd.h verdict
    assert set(cases) >= {"gap", "duplicate", "overlap", "balanced", "ack", "window", "option", "ttl", "tos", "df", "hlen", "thl",
                          "fin_mid", "psh_mid", "cwr_later", "syn", "rst", "urg", "p0", "dropped", "other_addr", "other_port"}
    r = b.run_gro_dev(dev)
    b.check_gro_dev(r)
    ref = b.run_gro_dev(dev, reference=True)                             # the same bytes and verdicts as today's way
    assert np.array_equal(ref["out"], r["out"]) and np.array_equal(ref["dverdict"], r["dverdict"])


# ---- 5. a mixed batch with no coalescible group ----
@pytest.mark.parametrize("align", [1, 16])
def test_mixed_batch_equals_the_existing_plan_and_build(dev, inet_oracle, align):
    frames = mixed_no_group(inet_oracle)
    b = GBatch(inet_oracle, frames, rr.F_TRAILER, align=align, lead=3, out_base=align & 3)
    assert not b.plan["merged"] and (b.fstat & rr.INCOMPLETE).any() and (b.dverdict & rd.L4_BAD_CSUM).any()
    r = b.run_gro_dev(dev)
    b.check_gro_dev(r)
    ref = b.run_gro_dev(dev, reference=True)
    for k in ("out", "dst", "dgi", "doff", "dlen", "dlead", "dverdict", "counts"):
        assert np.array_equal(r[k], ref[k]), k
    assert r["bad"] == ref["bad"]
    assert np.array_equal(r["fstat"] & ~np.uint32(gm.CAND), ref["fstat"]) and np.array_equal(r["final"] & ~np.uint32(gm.CAND), ref["final"])
    assert ((r["fstat"] & gm.CAND) != 0).sum() == 4


# ---- 7. room ----
def room_batch(inet_oracle, **kw):
    rng = np.random.default_rng(7)
    a = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 90), 10, sport=1), 40)       # 130 bytes merged
    lone = [mg.frame(gm.tcp_datagram(inet_oracle, payload(rng, 5), 77, sport=2), False)]       # 45 bytes
    c = cut(inet_oracle, gm.tcp_datagram(inet_oracle, payload(rng, 33), 500, sport=3), 11)      # 73 bytes merged
    return GBatch(inet_oracle, [a[1], lone[0], a[0], c[2], a[2], c[0], c[1]], bad_mask=rd.NO_ROOM | gm.GROD_MERGED, **kw)


def test_room_exact_one_short_and_none(dev, inet_oracle):
    full = room_batch(inet_oracle)
    assert full.m == 3 and full.plan["dlen"].tolist() == [45, 130, 73] and full.plan["dlead"].tolist() == [1, 2, 5]
    assert full.dverdict.tolist() == [TCP_OK, MERGED_WORD, MERGED_WORD] and full.bad == 2
    for out_bytes, fits in ((full.need, 3), (full.need - 1, 2), (45 + 129, 1), (44, 0), (0, 0)):
        b = room_batch(inet_oracle, out_bytes=out_bytes, out_base=3)
        assert b.dverdict[:fits].tolist() == full.dverdict[:fits].tolist() and (b.dverdict[fits:] == rd.NO_ROOM).all()
        assert ((b.fstat & rr.NO_ROOM) != 0).sum() == {3: 0, 2: 3, 1: 6, 0: 7}[fits]
        b.check_gro_dev(b.run_gro_dev(dev))                              # the canaries around `out` included


def test_no_frames_and_null_optional_outputs(dev, inet_oracle):
    b = GBatch(inet_oracle, [], 0)
    r = b.run_gro_dev(dev)
    assert r["counts"].tolist() == [0, 0] and np.array_equal(r["out"], b.expect) and r["bad"] == 0
    assert (r["dverdict"] == 0x55555555).all()
    assert na.rx_gro_host(b.arena, 0, b.off, b.ln, 0, b.out0, 0, None) == (0, 0)
    b = room_batch(inet_oracle, align=16)
    b.check_gro_dev(b.run_gro_dev(dev, bad=False, dlead=False, final=False), bad=False, dlead=False, final=False)


# ---- 8. the host form ----
def test_host_form_on_segmented_traffic_and_on_what_stays_apart(dev, inet_oracle):
    for mss, id_fixed in ((1460, False), (7, True)):
        b, dgs, _ = segmented_batch(dev, inet_oracle, mss, id_fixed, align=16)
        dv = b.check_gro_host()
        assert np.array_equal(dv, b.run_gro_dev(dev)["dverdict"][:b.m])
    frames, verdict, mask, _ = stays_apart(inet_oracle)
    GBatch(inet_oracle, frames, 0, verdict, mask, lead=1).check_gro_host()
    GBatch(inet_oracle, mixed_no_group(inet_oracle), rr.F_TRAILER, align=128).check_gro_host()


# ---- 9. scale and determinism (and the host form across a chunk cut) ----
@pytest.fixture(scope="module")
def scale(inet_oracle):
    """About 23 k frames of 200 interleaved flows: five 32 KiB windows each, cut at 1460, every 37th
    window with one segment lost; the slots fully permuted."""
    rng = np.random.default_rng(9)
    pay = payload(rng, 1 << 16)
    frames, lost = [], 0
    for f in range(200):
        for w in range(5):
            at = (f * 131 + w * 17) & 0x7FFF
            dg = gm.tcp_datagram(inet_oracle, pay[at:at + 32768 - 40], ((f * 7 + w) << 15) & 0xFFFFFFFF, src=0x0A000000 + f,
                                 sport=0x4000 + f, tflags=gm.ACK | (gm.PSH if w == 4 else 0))
            segs = cut(inet_oracle, dg, 1460, pad=0)
            if (f * 5 + w) % 37 == 0:
                del segs[1 + (f + w) % (len(segs) - 2)]                # a middle one: the rest does not tile
                lost += 1
            frames += segs
    order = rng.permutation(len(frames))
    b = GBatch(inet_oracle, [frames[i] for i in order], 0, align=16, out_base=2)
    return b, lost


def test_scale_and_determinism(dev, inet_oracle, scale):
    b, lost = scale
    assert 20000 < b.n < 24000 and lost == 28
    assert (b.dverdict == MERGED_WORD).sum() == 1000 - lost and b.m == 1000 - lost + lost * 22
    runs = [b.run_gro_dev(dev) for _ in range(2)]
    for r in runs:
        b.check_gro_dev(r)
    for k in ("out", "final", "dverdict", "dst", "dgi", "doff", "dlen", "dlead"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert assert_checksums(inet_oracle, b, runs[0]["out"]) == 1000 - lost


def test_host_form_across_a_chunk_cut(dev, inet_oracle, scale):
    b, _ = scale
    want = [e - k0 for k0, e, _frames, _bound in host_chunks(b.plan)]
    assert len(want) == 2                                                # the gathered frames exceed one chunk's staging
    b.check_gro_host(cut=want)


# ---- 10. launch names ----
def test_launch_names(dev, inet_oracle):
    b = room_batch(inet_oracle)
    b.check_gro_dev(b.run_gro_dev(dev))
    assert na.gro_last_launch() == "gro"
    before = (na.rxr_last_launch(), na.rxd_last_launch())
    b.run_gro_dev(dev)
    assert (na.rxr_last_launch(), na.rxd_last_launch()) == before       # the coalescing build is a launch of its own
    b.run_gro_dev(dev, reference=True)
    assert na.rxd_last_launch() == "general-l4" and na.gro_last_launch() == "gro"
