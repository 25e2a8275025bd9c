"""GPU tests of one-pass TCP segmentation (include/nstack_tso.h) through the C ABI. For every batch the
device form (after ip_tx_tso_plan_dev) and, where noted, the host form must leave output arenas equal to
the model's (tests/tso_model.py: byte surgery per segment, the oracle's checksum functions, then
tests/txf_model.py). The arena is canary bytes before, between and behind the slots and is compared as
a whole; flen, fcs, status, first and the planned status are compared with the model too. Where noted the
arena is also compared with ip_tx_frame_l4_dev run on the model-expanded datagrams placed at the same
slots. Every comparison is exact."""
import struct

import numpy as np
import pytest

import nstack_amd as na
import tso_model as tm
import txd_model as dm
import txf_model as fm
from tso_batch import TBatch, field, tcp_datagram
from txd_batch import DBatch, l4_datagram
from txf_batch import FCS, datagram, engine_constants, host_chunks, pack, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEG = tm.SEGMENTED | dm.L4_CSUM_SET | 6 << 16
ALL = tm.FIN | tm.PSH | tm.ACK | tm.ECE | tm.CWR


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def frame_at(b, arena, k):
    at = b.base + k * b.slot
    return arena[at:at + int(b.flen[k])].tobytes()


# ---- 1. alignments ----
@pytest.fixture(scope="module")
def aligned_dgs():
    rng = np.random.default_rng(601)
    return [tcp_datagram(rng, 20, thl, k * (1500 - 20 - thl) + t, tm.ACK | tm.PSH)
            for thl in (20, 32, 60) for k in (1, 2, 5) for t in range(1, 9)]


@pytest.mark.parametrize("base", range(4))
def test_segments_at_every_alignment(dev, oracle, inet_oracle, aligned_dgs, base):
    """mtu 1500, hlen 20, thl 20 / 32 / 60, P = k m + t for k = 1, 2, 5 and t = 1..8 (last segments of 1..8
    payload bytes); datagrams at alignments 0..3 against the output at `base`, in slots of 1518 (base 0, 2)
    or 1519 bytes (the destination's alignment changes slot by slot)."""
    n = len(aligned_dgs)
    b = TBatch(oracle, inet_oracle, aligned_dgs, 1500, FCS, base=base, seed=50 + base, slot=1518 + (base & 1),
               aligns=[(i + base + i // 4) & 3 for i in range(n)])
    assert {(int(o) & 3) for o in b.off} == {0, 1, 2, 3} and (b.status == SEG).all()
    assert sorted(set(np.diff(b.plan_first.astype(np.int64)))) == [2, 3, 6]
    res = b.run_dev(dev)
    b.check_dev(res)
    if base == 0:
        b.check_host()
    if base < 2:
        assert np.array_equal(res[0], b.expanded_way(oracle, inet_oracle, dev))


# ---- 2. odd and tiny units ----
def test_odd_and_tiny_units(dev, oracle, inet_oracle):
    """mss 1, 3, 7 with P <= 40 (every frame padded: hlen + thl + plen < 56) and 1459 (odd frames)."""
    rng = np.random.default_rng(602)
    dgs, mss = [], []
    for m in (1, 3, 7):
        for thl in (20, 24):
            for P in (m + 1, 2 * m, 15, 16, 39, 40):
                if P > m and 20 + thl + min(m, P) < 56:
                    dgs.append(tcp_datagram(rng, 20, thl, P, ALL))
                    mss.append(m)
    for P in (1460, 2918, 2919, 4377, 4378):
        dgs.append(tcp_datagram(rng, 20, 20, P, ALL))
        mss.append(1459)
    b = TBatch(oracle, inet_oracle, dgs, 1500, FCS, mss=mss, seed=60, slot=1519)
    assert (b.status == SEG).all() and (b.flen[:int(b.plan_first[-6])] == 70).all()
    assert {int(x) & 1 for x in b.flen[b.flen != 0xCCCCCCCC]} == {0, 1}
    res = b.run_dev(dev)
    b.check_dev(res)
    b.check_host()
    assert np.array_equal(res[0], b.expanded_way(oracle, inet_oracle, dev))
    TBatch(oracle, inet_oracle, dgs, 1500, 0, mss=mss, seed=61, slot=1515, base=1).check(dev)


# ---- 3. the three ways to give the mss ----
def test_mss_per_datagram_one_for_all_and_null(dev, oracle, inet_oracle):
    rng = np.random.default_rng(603)
    dgs = [tcp_datagram(rng, (20, 24)[q % 2], (20, 28, 40)[q % 3], P, ALL) for q, P in
           enumerate((100, 536, 537, 1072, 1400, 1420, 1461, 3000, 5000, 60, 1, 0))]
    per = [0, 536, 536, 1460, 100, 9000, 0, 65535, 1000, 59, 1, 1]
    a = TBatch(oracle, inet_oracle, dgs, 1500, FCS, mss=per, seed=62)
    o = TBatch(oracle, inet_oracle, dgs, 1500, FCS, mss=536, seed=62)
    z = TBatch(oracle, inet_oracle, dgs, 1500, FCS, mss=None, seed=62)
    assert o.flags & tm.F_MSS_ONE and not a.flags & tm.F_MSS_ONE
    # a datagram with D <= mtu but P > mss_i is segmented; without an mss it is whole
    assert a.status[4] == SEG and len(dgs[4]) <= 1500 and z.status[4] == fm.WHOLE | dm.L4_CSUM_SET | 6 << 16
    assert a.total > z.total and o.total > z.total and not np.array_equal(a.plan_first, o.plan_first)
    assert [bool(x) for x in z.segmented()] == [len(d) > 1500 for d in dgs]
    for b in (a, o, z):
        b.check(dev)
    # an all-zero mss array is the NULL array
    z0 = TBatch(oracle, inet_oracle, dgs, 1500, FCS, mss=[0] * len(dgs), seed=62)
    assert np.array_equal(z0.expect, z.expect)
    z0.check_dev(z0.run_dev(dev))


# ---- 4. wraps ----
def test_id_and_sequence_wrap(dev, oracle, inet_oracle):
    rng = np.random.default_rng(604)
    dgs = [tcp_datagram(rng, 20, 20, 5000, ALL, id0=0xFFFE, seq0=0xFFFFFFF0),
           tcp_datagram(rng, 24, 32, 4000, tm.ACK, id0=0xFFFF, seq0=0xFFFFFA4C - 1448),
           tcp_datagram(rng, 20, 20, 3000, tm.ACK, id0=7, seq0=0xFFFFFFFF)]
    for flags in (FCS, FCS | tm.F_ID_FIXED):
        b = TBatch(oracle, inet_oracle, dgs, 1500, flags, seed=63)
        res = b.run_dev(dev)
        b.check_dev(res)
        b.check_host()
        fr = [frame_at(b, res[0], k) for k in range(4)]
        assert [field(f, 20, "ip_id") for f in fr] == ([0xFFFE] * 4 if flags & tm.F_ID_FIXED else [0xFFFE, 0xFFFF, 0, 1])
        assert [field(f, 20, "seq") for f in fr] == [0xFFFFFFF0, 1460 - 16, 2920 - 16, 4380 - 16]
        assert np.array_equal(res[0], b.expanded_way(oracle, inet_oracle, dev))


# ---- 5. flags ----
def test_flags_of_first_middle_and_last_segment(dev, oracle, inet_oracle):
    rng = np.random.default_rng(605)
    dgs = [tcp_datagram(rng, h, t, 4000, ALL) for h, t in ((20, 20), (32, 20), (20, 44))]
    other = []
    for d in dgs:   # garbage in both checksum fields
        h = (d[0] & 15) * 4
        o = bytearray(d)
        for q in (10, 11, h + 16, h + 17):
            o[q] ^= 0xFF
        other.append(bytes(o))
    a = TBatch(oracle, inet_oracle, dgs, 1500, FCS, seed=64, aligns=[1, 2, 3])
    c = TBatch(oracle, inet_oracle, other, 1500, FCS, seed=64, aligns=[1, 2, 3])
    assert not np.array_equal(a.arena, c.arena) and np.array_equal(a.expect, c.expect)
    ra, rc = a.run_dev(dev), c.run_dev(dev)
    a.check_dev(ra)
    c.check_dev(rc)
    assert np.array_equal(ra[0], rc[0]) and np.array_equal(ra[2], rc[2])
    for i, d in enumerate(dgs):
        h, k = (d[0] & 15) * 4, int(a.plan_first[i])
        first, middle, last = (field(frame_at(a, ra[0], k + s), h, "flags") for s in range(3))
        assert first == tm.ACK | tm.ECE | tm.CWR and middle == tm.ACK | tm.ECE and last == tm.ACK | tm.ECE | tm.FIN | tm.PSH


# ---- 6. long headers ----
def test_long_headers_put_the_tcp_fields_into_the_second_image_dword(dev, oracle, inet_oracle):
    """hlen 24 + thl 60 and hlen 60 + thl 52 (112 bytes: the limit) are segmented; hlen 60 + thl 56 is not
    and falls to fragmentation. From hlen 32 on tcp_seqno, the flags and the checksum lie in frame dwords
    16 and up."""
    rng = np.random.default_rng(606)
    shapes = ((24, 60), (60, 52), (32, 20), (36, 40), (48, 60), (60, 56), (60, 20), (28, 24))
    dgs = [tcp_datagram(rng, h, t, P, ALL, seq0=0xFFFFF000) for h, t in shapes for P in (1500, 4001)]
    b = TBatch(oracle, inet_oracle, dgs, 1500, FCS, seed=65, aligns=[i & 3 for i in range(len(dgs))])
    want = [SEG if h + t <= 114 else fm.FRAGMENTED | dm.L4_CSUM_SET | 6 << 16 for h, t in shapes for _ in range(2)]
    assert list(b.status) == want and (14 + 32 + 4) // 4 >= 12 and (14 + 60 + 16) // 4 == 22
    res = b.run_dev(dev)
    b.check_dev(res)
    b.check_host()
    assert np.array_equal(res[0], b.expanded_way(oracle, inet_oracle, dev))
    TBatch(oracle, inet_oracle, dgs, 1500, 0, mss=333, seed=66, slot=1517, base=3).check(dev)


# ---- 7. segment bounds of the walk ----
def test_mtu_76(dev, oracle, inet_oracle):
    rng = np.random.default_rng(607)
    dgs = [tcp_datagram(rng, h, t, P, ALL) for h, t in ((20, 20), (20, 52), (24, 48), (36, 36), (20, 60), (60, 20))
           for P in (1, 17, 100, 333)]
    b = TBatch(oracle, inet_oracle, dgs, 76, FCS, seed=67)
    assert (b.status & tm.SEGMENTED).sum() >= 12 and (b.status & (fm.FRAGMENTED | fm.WHOLE)).any()
    b.check(dev)
    TBatch(oracle, inet_oracle, dgs, 76, 0, seed=68, slot=91, base=3).check(dev)


@pytest.mark.parametrize("mtu", [1522, 1523])
def test_frames_of_one_and_of_two_walk_segments(dev, oracle, inet_oracle, mtu):
    """mtu 1522: full frames of 1536 bytes, one 1536-byte walk segment. mtu 1523: 1537 bytes, two walk
    segments, so every full frame takes the sum-only first visit."""
    rng = np.random.default_rng(608)
    dgs = [tcp_datagram(rng, h, t, P, ALL) for h, t in ((20, 20), (24, 32), (20, 60), (60, 52))
           for P in (mtu - h - t + 1, 2 * (mtu - h - t), 3 * (mtu - h - t) + 7)]
    b = TBatch(oracle, inet_oracle, dgs, mtu, FCS, seed=69, slot=14 + mtu + 4 + (mtu & 1))
    assert (b.status == SEG).all() and int(b.flen[b.flen != 0xCCCCCCCC].max()) == 14 + mtu
    res = b.run_dev(dev)
    b.check_dev(res)
    b.check_host()
    assert np.array_equal(res[0], b.expanded_way(oracle, inet_oracle, dev))


@pytest.mark.parametrize("flags", [FCS, 0])
def test_mtu_9000(dev, oracle, inet_oracle, flags):
    rng = np.random.default_rng(609)
    dgs = [tcp_datagram(rng, h, t, P, ALL) for (h, t), P in zip(((20, 20), (24, 32), (20, 60), (60, 52), (20, 20), (20, 24)),
                                                                (8961, 17920, 20001, 30000, 65535 - 40, 9100))]
    mss = [0, 0, 0, 8001, 0, 1537]
    b = TBatch(oracle, inet_oracle, dgs, 9000, flags, mss=mss, seed=70, base=1)
    assert (b.status == SEG).all()
    b.check(dev, host=bool(flags))


def test_the_largest_datagram_at_mtu_1500(dev, oracle, inet_oracle):
    rng = np.random.default_rng(610)
    b = TBatch(oracle, inet_oracle, [tcp_datagram(rng, 20, 20, 65535 - 40, ALL)], 1500, FCS, seed=71)
    assert b.total == 45 and na.tx_tso_count(65535, 20, 20, ALL, 0, 0, 1500) == 45
    b.check(dev)


# ---- 8. mixed runs ----
def mixed_dgs(rng, n=40):
    """Segmented TCP, whole TCP, fragmented UDP, ICMP and SYN-over-mtu in turn, in sizes that put several
    into one row's run of eight."""
    dgs = []
    for q in range(n):
        kind = q % 5
        if kind == 0:
            dgs.append(tcp_datagram(rng, (20, 24, 60)[q % 3], (20, 32, 52)[(q // 5) % 3], 1500 + 700 * (q % 7), ALL))
        elif kind == 1:
            dgs.append(tcp_datagram(rng, 20, (20, 40)[q % 2], (37 * q) % 1400, tm.ACK | tm.PSH))
        elif kind == 2:
            dgs.append(l4_datagram(rng, 17, (20, 28)[q % 2], 1600 + 450 * (q % 6)))
        elif kind == 3:
            dgs.append(l4_datagram(rng, 1, 20, (64, 1472, 3000)[q % 3]))
        else:
            dgs.append(tcp_datagram(rng, 20, 20, 2000 + 100 * q, tm.SYN | tm.ACK))
    return dgs


def test_mixed_runs(dev, oracle, inet_oracle):
    dgs = mixed_dgs(np.random.default_rng(611))
    for mtu in (1500, 9000):
        b = TBatch(oracle, inet_oracle, dgs, mtu, FCS, seed=72 + mtu, slot=14 + mtu + 4 + 1)
        seen = int(np.bitwise_or.reduce(b.status)) & 0xFFFF
        assert seen == (tm.SEGMENTED if mtu == 1500 else 0) | fm.WHOLE | (fm.FRAGMENTED if mtu == 1500 else 0) | dm.L4_CSUM_SET
        res = b.run_dev(dev)
        b.check_dev(res)
        b.check_host()
        assert np.array_equal(res[0], b.expanded_way(oracle, inet_oracle, dev))


def test_refused_datagrams_and_no_room_between_live_ones(dev, oracle, inet_oracle):
    rng = np.random.default_rng(612)
    mtu = 1500
    bad = [b"", rng.integers(0, 256, 19, dtype=np.uint8).tobytes(), datagram(rng, 20, 30, vhl=0x05, proto=6),
           datagram(rng, 24, 17, ip_len=40, proto=6), tcp_datagram(rng, 20, 20, 3000, tm.ACK, foff=0x2000),
           tcp_datagram(rng, 28, 20, 2 * mtu, tm.ACK, foff=0x0003), tcp_datagram(rng, 20, 20, 3000, tm.SYN, foff=0x4000),
           tcp_datagram(rng, 20, 20, 200, tm.ACK, foff=0x2000)]
    dgs = []
    for q, d in enumerate(mixed_dgs(rng)):
        dgs += [d, bad[q % 8]]
    b = TBatch(oracle, inet_oracle, dgs, mtu, FCS | fm.F_HONOR_DF, seed=73, slot=1519)
    seen = int(np.bitwise_or.reduce(b.status)) & 0xFFFF
    assert seen == (tm.SEGMENTED | fm.WHOLE | fm.FRAGMENTED | fm.BAD_HDR | fm.BAD_LEN | fm.REFRAG | fm.DF_DROP |
                    dm.L4_CSUM_SET)
    b.check(dev)
    # TXF_NO_ROOM: slots run out in the middle; nothing of those datagrams is written
    first = b.plan_first.copy()
    first[30:] += 13                                                    # a hole, then past the end for the last ones
    r = TBatch(oracle, inet_oracle, dgs, mtu, FCS | fm.F_HONOR_DF, seed=73, slot=1519, first=first[:-1], slots=b.slots)
    no_room = (r.status & fm.NO_ROOM) != 0
    assert no_room.any() and not no_room[:30].any() and (r.status[no_room] & tm.SEGMENTED).any()
    assert ((r.status[no_room] & (dm.L4_CSUM_SET | dm.L4_SHORT)) == 0).all()
    r.check_dev(r.run_dev(dev))


# ---- 9. nothing segmentable: ip_tx_frame_l4_dev's bytes ----
def test_a_batch_with_nothing_segmentable_equals_ip_tx_frame_l4_dev(dev, oracle, inet_oracle):
    rng = np.random.default_rng(613)
    dgs = [l4_datagram(rng, (17, 1)[q % 2], (20, 24, 60)[q % 3], L) for q, L in enumerate((0, 30, 999, 1480, 3000, 10000))]
    dgs += [tcp_datagram(rng, 20, 20, P, fl, foff=fo) for P, fl, fo in
            ((1460, ALL, 0), (100, ALL, 0), (3000, tm.SYN, 0), (3000, tm.ACK | tm.RST, 0), (3000, tm.ACK | tm.URG, 0),
             (300, ALL, 0x2000), (4000, ALL, 0x4000 | 5))]
    dgs += [tcp_datagram(rng, 60, 56, 3000, ALL), l4_datagram(rng, 6, 20, 19), l4_datagram(rng, 6, 20, 7000)[:20 + 7000]]
    o = bytearray(dgs[-1])
    o[20 + 12] = 0x40                                                    # thl 16
    dgs[-1] = bytes(o)
    for flags in (FCS, dm.F_UDP_ZERO):
        b = TBatch(oracle, inet_oracle, dgs, 1500, flags, seed=74, aligns=[i & 3 for i in range(len(dgs))])
        assert not b.segmented().any()
        res = b.run_dev(dev)
        b.check_dev(res)
        out_d, st_d = b.run_txd_dev(dev)
        assert np.array_equal(res[0], out_d) and np.array_equal(res[3], st_d) and np.array_equal(out_d, b.txd_expect)


# ---- 10. round trip ----
def test_every_segment_frame_passes_ether_rx_validate_dev(dev, oracle, inet_oracle):
    rng = np.random.default_rng(614)
    dgs = [tcp_datagram(rng, h, t, P, ALL) for (h, t), P in zip(((20, 20), (24, 32), (20, 60), (60, 52), (20, 20), (20, 24), (20, 20)),
                                                                (1461, 3000, 4381, 2777, 30, 45, 20000))]
    b = TBatch(oracle, inet_oracle, dgs, 1500, FCS, mss=[0, 0, 1459, 0, 7, 11, 0], seed=75)
    assert (b.status == SEG).all()
    out = b.run_dev(dev)[0]
    off = (b.base + np.arange(b.slots, dtype=np.uint64) * np.uint64(b.slot)).astype(np.uint64)
    ln = (b.flen + 4).astype(np.uint32)
    d_v = torch.zeros(b.slots, dtype=torch.int32, device=dev)
    na.rx_validate_dev(to_dev(out, dev), out.size, to_dev(off, dev), to_dev(ln, dev), d_v, b.slots, na.RXV_F_TRAILER)
    torch.cuda.synchronize()
    v = d_v.cpu().numpy().view(np.uint32)
    padded = np.array([struct.unpack_from(">H", frame_at(b, out, k), 16)[0] < 56 for k in range(b.slots)])
    assert padded.sum() >= 9 and (~padded).sum() >= 20
    assert (v & na.RXV_L4_CHECKED != 0).all() and (v & (na.RXV_FRAG | na.RXV_L4_BAD_CSUM) == 0).all()
    ok = na.RXV_IPV4 | na.RXV_L4_CHECKED | 6 << na.RXV_PROTO_SHIFT
    assert (v[~padded] == ok).all() and (v[padded] == ok | na.RXV_IP_BAD_LEN).all(), [hex(x) for x in v[:8]]


# ---- 11. the host form across three chunks ----
def test_host_form_across_three_chunks_cut_by_datagram_bytes(dev, oracle, inet_oracle):
    """1030 TCP datagrams of 65535 bytes at mtu 9000 (eight segments each), three distinct ones gathered
    through repeated off[]: 512 of them fill a chunk's 32 MiB of datagrams. The mss entries travel per chunk."""
    rng, mtu, n = np.random.default_rng(615), 9000, 1030
    pool = [tcp_datagram(rng, h, t, 65535 - h - t, ALL) for h, t in ((20, 20), (36, 32), (60, 52))]
    arena, poff, pln = pack(pool, seed=616)
    pick = rng.integers(0, 3, n)
    mss = np.where(np.arange(n) % 2 == 0, 0, 8900).astype(np.uint16)
    b = TBatch(oracle, inet_oracle, None, mtu, FCS, mss=mss, placed=(arena, poff[pick], pln[pick]),
               l2=np.random.default_rng(617).integers(0, 256, (2, 12), dtype=np.uint8)[rng.integers(0, 2, n)], seed=76)
    chunks = host_chunks(b.plan_first, b.ln, b.slot, engine_constants())
    assert [(e - i, bound) for i, e, _, bound in chunks] == [(512, "in"), (512, "in"), (6, "end")]
    assert b.total == 8 * n and (b.status == SEG).all()
    b.check_host()


def test_host_form_across_three_chunks_cut_by_slots(dev, oracle, inet_oracle):
    """Eight datagrams of 300 payload bytes at mss 1 (300 frames each) in slots of 64 KiB: three of them fill
    a chunk's 64 MiB of slots."""
    rng = np.random.default_rng(618)
    pool = [tcp_datagram(rng, 20, t, 300, ALL) for t in (20, 32)]
    arena, poff, pln = pack(pool, seed=619)
    pick = np.array([0, 1, 1, 0, 0, 1, 0, 1])
    b = TBatch(oracle, inet_oracle, None, 1500, FCS | fm.F_L2_ONE, mss=1, placed=(arena, poff[pick], pln[pick]),
               l2=np.random.default_rng(620).integers(0, 256, (8, 12), dtype=np.uint8), seed=77, slot=65536)
    chunks = host_chunks(b.plan_first, b.ln, b.slot, engine_constants())
    assert [(e - i, bound) for i, e, _, bound in chunks] == [(3, "out"), (3, "out"), (2, "end")]
    assert b.total == 2400 and b.flags & tm.F_MSS_ONE
    b.check_host()


# ---- 12. unchanged behaviour ----
def test_launch_names_in_the_same_process(dev, oracle, inet_oracle):
    rng = np.random.default_rng(621)
    dgs = [tcp_datagram(rng, 20, 20, P, ALL) for P in (0, 999, 3000, 10000)] + [l4_datagram(rng, 17, 20, 4000)]
    for flags, name, l4, plain in ((FCS, "tso-fcs", "general-l4-fcs", "general-fcs"), (0, "tso", "general-l4", "general")):
        b = TBatch(oracle, inet_oracle, dgs, 1500, flags, seed=78)
        out_f, st_f = b.run_txf_dev(dev)
        out_d, _ = b.run_txd_dev(dev)
        assert (na.txf_last_launch(), na.txd_last_launch()) == (plain, l4)
        b.check_dev(b.run_dev(dev))
        assert (na.tso_last_launch(), na.txf_last_launch(), na.txd_last_launch()) == (name, plain, l4)
        out_f2, st_f2 = b.run_txf_dev(dev)
        out_d2, _ = b.run_txd_dev(dev)
        assert na.tso_last_launch() == name
        assert np.array_equal(out_f, b.txf_expect) and np.array_equal(out_f2, b.txf_expect)
        assert np.array_equal(st_f, b.txf_status) and np.array_equal(st_f2, b.txf_status)
        assert np.array_equal(out_d, b.txd_expect) and np.array_equal(out_d2, b.txd_expect)
        assert not np.array_equal(b.txd_expect, b.expect)


# ---- 13. no fallback ----
def test_host_counters_stay_untouched(dev, oracle, inet_oracle):
    L = na.load()
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    rng = np.random.default_rng(622)
    b = TBatch(oracle, inet_oracle, [tcp_datagram(rng, 20, 20, 5000), l4_datagram(rng, 17, 24, 100)], 1500, FCS, seed=79)
    b.check(dev)
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before


# ---- 14. the plan's scan at the block borders and past one pass of the totals scan ----
@pytest.mark.parametrize("n", [255, 256, 257, 65537])
def test_plan_prefix_sums(dev, inet_oracle, n):
    """n tiny TCP datagrams of a few kinds (segmented into 2..8 frames, whole, SYN, UDP, refused) at every
    alignment: first[] and status[] of ip_tx_tso_plan_dev against tso_model, one model call per kind."""
    rng = np.random.default_rng(700 + n)
    kinds = [(tcp_datagram(rng, 20, 20, P, ALL), m) for P, m in ((2, 1), (8, 1), (7, 3), (5, 2), (8, 3), (4, 4), (0, 1))]
    kinds += [(tcp_datagram(rng, 24, 24, 6, tm.ACK), 2), (tcp_datagram(rng, 20, 20, 6, tm.SYN), 1),
              (l4_datagram(rng, 17, 20, 9), 1), (bytes(7), 1)]
    k_st, k_first = tm.plan_status(inet_oracle, [d for d, _ in kinds], 1500, 0, [m for _, m in kinds])
    k_cnt = np.diff(k_first)
    assert sorted(set(int(c) for c in k_cnt)) == [0, 1, 2, 3, 8] and (k_st & tm.SEGMENTED).any() and (k_st & fm.BAD_HDR).any()
    pick = rng.integers(0, len(kinds), n)
    ln = np.array([len(d) for d, _ in kinds], dtype=np.uint32)[pick]
    end = np.cumsum(ln.astype(np.uint64) + rng.integers(0, 4, n).astype(np.uint64))   # gaps of 0..3: every alignment
    off = (end - ln).astype(np.uint64)
    arena = np.zeros(int(end[-1]) + 8, dtype=np.uint8)
    for k, (d, _) in enumerate(kinds):
        at = off[pick == k]
        arena[(at[:, None] + np.arange(len(d), dtype=np.uint64)).astype(np.int64)] = np.frombuffer(d, dtype=np.uint8)
    mss = np.array([m for _, m in kinds], dtype=np.uint16)[pick]
    want = np.zeros(n + 1, dtype=np.uint64)
    want[1:] = np.cumsum(k_cnt[pick])
    d_arena = to_dev(arena, dev)
    d_first = torch.full((n + 1,), -1, dtype=torch.int64, device=dev)
    d_st = torch.full((n,), -1, dtype=torch.int32, device=dev)
    na.tx_tso_plan_dev(d_arena, arena.size, to_dev(off, dev), to_dev(ln, dev), to_dev(mss.view(np.int16), dev), n, 1500,
                       d_first, 0, d_st)
    torch.cuda.synchronize()
    assert (d_first.cpu().numpy().view(np.uint64) == want).all()
    assert (d_st.cpu().numpy().view(np.uint32) == k_st[pick]).all()
