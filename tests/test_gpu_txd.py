"""GPU tests of TX framing with L4 checksums (include/nstack_txd.h) through the C ABI. For every batch
the device form (after ether_tx_frame_plan_dev) and the host form must leave output arenas equal to
the model's (tests/txd_model.py: the oracle's checksum functions fill the field, tests/txf_model.py
frames the result). The arena is canary bytes before, between and behind the slots and is compared
as a whole; flen, fcs, status and first are compared with the model too. Every comparison is exact."""
import struct

import numpy as np
import pytest

import nstack_amd as na
import rxd_model as rd
import txd_model as dm
import txf_model as fm
from rxd_batch import DBatch as RxBatch
from txd_batch import FCS, DBatch, l4_datagram, udp_summing_to_zero
from txf_batch import datagram, engine_constants, host_chunks, pack, to_dev

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PROTOS = (6, 17, 1)
HLENS = (20, 24, 60)
FIELD = dm.L4_FIELD


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def field_frames(b):
    """[(datagram, fragment that holds its field, frame bytes without the FCS)] of a batch, from the model."""
    buf, out = b.arena.tobytes(), []
    for i in range(b.n):
        dg = buf[int(b.off[i]):int(b.off[i]) + int(b.ln[i])]
        q = dm.field_fragment(dg, b.mtu, b.flags)
        if q is not None and not int(b.status[i]) & fm.NO_ROOM:
            out.append((i, q, int(b.flen[int(b.plan_first[i]) + q])))
    return out


# ---- 1. whole datagrams ----
@pytest.fixture(scope="module")
def whole_dgs():
    rng = np.random.default_rng(501)
    dgs = [l4_datagram(rng, p, h, L) for p in PROTOS for h in HLENS for L in range(0, 41)]
    dgs += [l4_datagram(rng, PROTOS[q % 3], HLENS[q % 3 if q % 2 else (q // 3) % 3], int(rng.integers(0, 1500 - 60 + 1)))
            for q in range(300)]
    dgs += [l4_datagram(rng, p, h, 1500 - h) for p in PROTOS for h in HLENS]      # the largest whole frames
    return dgs


@pytest.mark.parametrize("base", range(4))
def test_whole_datagrams_at_every_alignment(dev, oracle, inet_oracle, whole_dgs, base):
    """Three protocols x three header lengths, L = 0..40 (every short bound and its neighbours), 300
    random lengths; the datagrams at alignments 0..3 against the output at `base`, in slots of 1522
    (base 0, 2) or 1523 bytes (no multiple of 4: the destination's alignment changes slot by slot)."""
    n = len(whole_dgs)
    b = DBatch(oracle, inet_oracle, whole_dgs, 1500, FCS, base=base, seed=20 + base, slot=1522 + (base & 1),
               aligns=[(i + base + i // 4) & 3 for i in range(n)])
    assert {(int(o) & 3) for o in b.off} == {0, 1, 2, 3} and (b.status & fm.WHOLE).all()
    seen = int(np.bitwise_or.reduce(b.status)) & 0xFFFF
    assert seen == fm.WHOLE | dm.L4_CSUM_SET | dm.L4_SHORT
    res = b.run_dev(dev)
    b.check_dev(res)
    if base == 0:
        b.check_host()
    if base < 2:   # framing, then sealing: two passes give the same bytes
        out, _ = b.run_txf_dev(dev)
        d_out = to_dev(out, dev)
        off = (b.base + np.arange(b.slots, dtype=np.uint64) * np.uint64(b.slot)).astype(np.uint64)
        na.tx_seal_dev(d_out, out.size, to_dev(off, dev), to_dev(b.flen, dev), b.slots, na.TXS_F_FCS)
        torch.cuda.synchronize()
        sealed = d_out.cpu().numpy()
        diff = np.flatnonzero(sealed != res[0])
        assert diff.size == 0, (diff[:8], [(int(d) - b.base) // b.slot for d in diff[:8]])


# ---- 2. fragmented datagrams ----
def test_fragmented_at_mtu_1500(dev, oracle, inet_oracle):
    """2, 3 and 6 fragments with last fragments of 1..8 payload bytes (odd and even D) and a few
    lengths in between, every protocol and header length."""
    rng = np.random.default_rng(502)
    dgs = []
    for q, (p, h) in enumerate((p, h) for p in PROTOS for h in HLENS):
        mx = fm.frag_unit(1500, h)
        for c in (2, 3, 6):
            for t in range(1, 9):   # hlen + max + 8 <= mtu: two fragments begin at a last fragment of 9 bytes
                if (t + q + c) % 3 == 0 or c == 2:
                    dgs.append(l4_datagram(rng, p, h, (c - 1) * mx + (t + 8 if c == 2 else t)))
            dgs.append(l4_datagram(rng, p, h, int(rng.integers((c - 1) * mx + 9, c * mx + 1))))
    b = DBatch(oracle, inet_oracle, dgs, 1500, FCS, seed=31)
    cnt = np.diff(b.plan_first.astype(np.int64))
    assert set(cnt) == {2, 3, 6} and (b.status & fm.FRAGMENTED).all() and (b.status & dm.L4_CSUM_SET).all()
    assert {int(x) & 1 for x in b.ln} == {0, 1}
    assert all(q == 0 for _, q, _ in field_frames(b))
    b.check(dev)
    b0 = DBatch(oracle, inet_oracle, dgs[::3], 1500, 0, seed=32, slot=1515)
    b0.check(dev)


def test_small_units_put_the_field_into_a_later_fragment(dev, oracle, inet_oracle):
    """mtu 76: hlen 20, 52 and 60 give units of 48, 16 and 8 bytes, so the TCP field (segment bytes
    16, 17) lies in fragment 0, 1 and 2; UDP's (6, 7) and ICMP's (2, 3) stay in fragment 0."""
    rng = np.random.default_rng(503)
    dgs, want = [], []
    for h, q in ((20, 0), (52, 1), (60, 2)):
        for L in (57, 60, 100, 101, 333, 1000):
            for p in PROTOS:
                dgs.append(l4_datagram(rng, p, h, L))
                want.append(q if p == 6 else 0)
    b = DBatch(oracle, inet_oracle, dgs, 76, FCS, seed=33)
    assert [q for _, q, _ in field_frames(b)] == want and (b.status & fm.FRAGMENTED).all()
    assert [fm.frag_unit(76, h) for h in (20, 52, 60)] == [48, 16, 8]
    b.check(dev)
    DBatch(oracle, inet_oracle, dgs, 76, 0, seed=34, slot=91, base=3).check(dev)


# ---- 3. field frames of several segments ----
def jumbo_dgs(rng):
    """Whole frames of F = 1536 k + t (k = 1, 2; t = -4..4), F = 1561..1627 (every relation of the three
    field positions and of 14 + hlen to the border between the front segment and the next), 9014 and
    65535 + 14 bytes."""
    Fs = [1536 * k + t for k in (1, 2) for t in range(-4, 5)] + list(range(1561, 1628, 3)) + [1570, 1571, 1612, 1613]
    dgs = []
    for q, F in enumerate(Fs):
        p, h = PROTOS[q % 3], HLENS[(q // 3) % 3]
        dgs.append(l4_datagram(rng, p, h, F - 14 - h))
    for p in PROTOS:   # the front segment ends inside or just behind the field
        for h in HLENS:
            for d in (-1, 0, 1, 2, 3):
                dgs.append(l4_datagram(rng, p, h, 1536 + FIELD[p] + d))   # F - 1536 = 14 + h + field + d
    dgs += [l4_datagram(rng, 17, 20, 9000 - 20), l4_datagram(rng, 6, 24, 9000 - 24), l4_datagram(rng, 1, 60, 65535 - 60),
            l4_datagram(rng, 6, 20, 65535 - 20)]
    return dgs


@pytest.mark.parametrize("flags", [FCS, 0])
def test_whole_frames_of_several_segments(dev, oracle, inet_oracle, flags):
    dgs = jumbo_dgs(np.random.default_rng(504))
    b = DBatch(oracle, inet_oracle, dgs, 65535, flags, seed=35, base=1)
    assert (b.status & fm.WHOLE).all() and (b.status & dm.L4_CSUM_SET).all()
    fl = {F for _, _, F in field_frames(b)}
    assert {1532, 1536, 1537, 1540, 3068, 3072, 3073, 3076, 9014, 65549} <= fl
    b.check(dev, host=bool(flags))


@pytest.mark.parametrize("flags", [FCS, 0])
def test_fragmented_at_mtu_9000(dev, oracle, inet_oracle, flags):
    """The head fragment (8986 or 8994 bytes) has six segments and holds the field."""
    rng = np.random.default_rng(505)
    dgs = [l4_datagram(rng, PROTOS[q % 3], HLENS[q % 3], L) for q, L in
           enumerate((8981, 9000, 12345, 17961, 17969, 30001, 65535 - 60, 8985, 26000))]
    b = DBatch(oracle, inet_oracle, dgs, 9000, flags, seed=36)
    assert (b.status & fm.FRAGMENTED).all() and all(q == 0 and F > 8900 for _, q, F in field_frames(b))
    b.check(dev, host=bool(flags))


# ---- 4. field values ----
def test_field_garbage_is_ignored_and_special_values(dev, oracle, inet_oracle):
    rng = np.random.default_rng(506)
    dgs = [l4_datagram(rng, p, h, L) for p in PROTOS for h in HLENS for L in (64, 2000, 2999)]
    dgs += [udp_summing_to_zero(inet_oracle, rng, h, n) for h in HLENS for n in (2, 31, 1700)]
    zero_icmp = [l4_datagram(rng, 1, h, L, seg=bytes(L)) for h in HLENS for L in (4, 8, 1999)]
    dgs += zero_icmp
    other = []
    for d in dgs:
        h, p = (d[0] & 15) * 4, d[9]
        o = bytearray(d)
        o[h + FIELD[p]:h + FIELD[p] + 2] = bytes(x ^ 0xFF for x in d[h + FIELD[p]:h + FIELD[p] + 2])
        other.append(bytes(o))
    aligns = [i & 3 for i in range(len(dgs))]
    a = DBatch(oracle, inet_oracle, dgs, 1500, FCS, seed=37, aligns=aligns)
    c = DBatch(oracle, inet_oracle, other, 1500, FCS, seed=37, aligns=aligns)
    assert not np.array_equal(a.arena, c.arena) and np.array_equal(a.expect, c.expect)
    ra, rc = a.run_dev(dev), c.run_dev(dev)
    a.check_dev(ra)
    c.check_dev(rc)
    assert np.array_equal(ra[0], rc[0]) and np.array_equal(ra[2], rc[2])
    # what the model stored: 0xffff for the UDP sums of 0, ip_checksum's own answer for the all-zero ICMP message
    for i in range(27, 36):
        k, h = int(a.plan_first[i]), (dgs[i][0] & 15) * 4
        at = a.base + k * a.slot + 14 + h + 6
        assert a.expect[at:at + 2].tobytes() == b"\xff\xff", i
    for i in range(36, 45):
        k, h = int(a.plan_first[i]), (dgs[i][0] & 15) * 4
        at, L = a.base + k * a.slot + 14 + h + 2, len(dgs[i]) - h
        assert a.expect[at:at + 2].tobytes() == struct.pack("<H", inet_oracle.oracle_ip_checksum(bytes(L), L)), i
    # TXD_F_UDP_ZERO: the UDP fields are 0, L4_CSUM_SET clear for them and set for the others
    z = DBatch(oracle, inet_oracle, dgs, 1500, FCS | dm.F_UDP_ZERO, seed=38, aligns=aligns)
    udp = np.array([d[9] == 17 for d in dgs])
    assert ((z.status[udp] & dm.L4_CSUM_SET) == 0).all() and ((z.status[~udp] & dm.L4_CSUM_SET) != 0).all()
    for i in np.flatnonzero(udp):
        at = z.base + int(z.plan_first[i]) * z.slot + 14 + (dgs[i][0] & 15) * 4 + 6
        assert z.expect[at:at + 2].tobytes() == b"\x00\x00"
    z.check(dev)


# ---- 5. neighbours ----
def test_refused_fragment_inputs_and_no_room_between_live_ones(dev, oracle, inet_oracle):
    rng = np.random.default_rng(507)
    mtu = 1500
    bad = [b"", rng.integers(0, 256, 19, dtype=np.uint8).tobytes(), datagram(rng, 20, 30, vhl=0x05, proto=6),
           datagram(rng, 24, 17, ip_len=40, proto=17), datagram(rng, 20, mtu, foff=0x2000, proto=6),
           datagram(rng, 28, 2 * mtu, foff=0x0003, proto=17), datagram(rng, 20, 3000, foff=0x4000, proto=1)]
    frag_in = [l4_datagram(rng, p, h, 200, foff=f) for p in PROTOS for h, f in ((20, 0x2000), (24, 0x00B9), (60, 0x2001))]
    dgs = []
    for q in range(40):
        dgs.append(l4_datagram(rng, PROTOS[q % 3], HLENS[q % 3], (37 * q) % 1400 if q % 4 else 1600 + 100 * q))
        dgs.append(bad[q % 7] if q % 2 else frag_in[q % 9])
    b = DBatch(oracle, inet_oracle, dgs, mtu, FCS | fm.F_HONOR_DF, seed=39, slot=1519)
    seen = int(np.bitwise_or.reduce(b.status))
    assert seen & 0xFFFF == fm.WHOLE | fm.FRAGMENTED | fm.BAD_HDR | fm.BAD_LEN | fm.REFRAG | fm.DF_DROP | dm.L4_CSUM_SET
    # a fragment input framed whole: ether_tx_frame_dev's bytes, protocol bits only
    out_f, _ = b.run_txf_dev(dev)
    for i in range(1, 80, 2):
        if dgs[i] in frag_in:
            k = int(b.plan_first[i])
            at = b.base + k * b.slot
            assert b.status[i] == fm.WHOLE | (dgs[i][9] << 16)
            assert np.array_equal(b.expect[at:at + b.slot], out_f[at:at + b.slot])
    b.check(dev)
    # TXF_NO_ROOM: slots run out in the middle; nothing of those datagrams is written
    first = b.plan_first.copy()
    first[30:] += 5                                                     # a hole, then past the end for the last ones
    r = DBatch(oracle, inet_oracle, dgs, mtu, FCS | fm.F_HONOR_DF, seed=39, slot=1519, first=first[:-1], slots=b.slots)
    assert (r.status & fm.NO_ROOM).any() and not (r.status[:30] & fm.NO_ROOM).any()
    assert ((r.status[(r.status & fm.NO_ROOM) != 0] & (dm.L4_CSUM_SET | dm.L4_SHORT)) == 0).all()
    r.check_dev(r.run_dev(dev))


def test_runs_of_alternating_protocol_and_size(dev, oracle, inet_oracle):
    """40 consecutive live datagrams, protocol and size alternating, so that a row frames eight in a run:
    a sum or a delta carried over from the datagram before shows at once."""
    rng = np.random.default_rng(508)
    sizes = (1, 1400, 4000, 20, 700, 9000, 64, 2900)
    dgs = [l4_datagram(rng, PROTOS[q % 3], HLENS[(q // 2) % 3], 20 + sizes[q % 8]) for q in range(40)]
    for mtu in (1500, 9000):
        b = DBatch(oracle, inet_oracle, dgs, mtu, FCS, seed=40 + mtu)
        assert (b.status & dm.L4_CSUM_SET).all()
        b.check(dev)


# ---- 6. round trip on the device ----
def test_round_trip_through_validation_and_reassembly(dev, oracle, inet_oracle):
    rng = np.random.default_rng(509)
    dgs = [l4_datagram(rng, PROTOS[q % 3], HLENS[(q // 3) % 3], L) for q, L in
           enumerate((20, 21, 56, 300, 1480, 1481, 2000, 2944, 2945, 4000, 7000, 9000, 100, 8, 1473, 64))]
    for q, d in enumerate(dgs):   # distinct ids, so that reassembly keeps the datagrams apart
        o = bytearray(d)
        o[4:6] = (0x1000 + q).to_bytes(2, "big")
        dgs[q] = bytes(o)
    b = DBatch(oracle, inet_oracle, dgs, 1500, FCS, seed=41)
    out = b.run_dev(dev)[0]
    b.check_dev(b.run_dev(dev))
    off = (b.base + np.arange(b.slots, dtype=np.uint64) * np.uint64(b.slot)).astype(np.uint64)
    ln = (b.flen + 4).astype(np.uint32)
    d_v = torch.zeros(b.slots, dtype=torch.int32, device=dev)
    na.rx_validate_dev(to_dev(out, dev), out.size, to_dev(off, dev), to_dev(ln, dev), d_v, b.slots, na.RXV_F_TRAILER)
    torch.cuda.synchronize()
    v = d_v.cpu().numpy().view(np.uint32)
    defects = na.RXV_FCS_BAD | na.RXV_RUNT | na.RXV_IP_BAD_HDR | na.RXV_IP_BAD_CSUM | na.RXV_L4_BAD_CSUM | na.RXV_L4_SHORT
    assert (v & defects == 0).all() and (v & na.RXV_IPV4 != 0).all(), [hex(x) for x in v[:8]]
    rx = RxBatch(inet_oracle, flags=na.RXR_F_TRAILER, placed=(out, off, ln), seed=42)
    assert rx.m == len(dgs)
    r = rx.run_l4_dev(dev)
    rx.check_l4_dev(r)
    got = r["dverdict"][:rx.m]
    assert (got & rd.L4_CHECKED != 0).all() and (got & (rd.L4_BAD_CSUM | rd.L4_SHORT) == 0).all() and r["bad"] == 0


# ---- 7. the host form across three chunks ----
def test_host_form_across_three_chunks(dev, oracle, inet_oracle):
    """1030 UDP / TCP / ICMP datagrams of 65535 bytes at mtu 9000, three distinct ones gathered through
    repeated off[]: 512 of them fill a chunk's 32 MiB of datagrams."""
    rng, mtu, n = np.random.default_rng(510), 9000, 1030
    pool = [l4_datagram(rng, p, h, 65535 - h) for p, h in zip(PROTOS, (20, 36, 60))]
    arena, poff, pln = pack(pool, seed=511)
    pick = rng.integers(0, 3, n)
    b = DBatch(oracle, inet_oracle, None, mtu, FCS, placed=(arena, poff[pick], pln[pick]),
               l2=np.random.default_rng(512).integers(0, 256, (2, 12), dtype=np.uint8)[rng.integers(0, 2, n)], seed=43)
    k = engine_constants()
    chunks = host_chunks(b.plan_first, b.ln, b.slot, k)
    assert [(e - i, bound) for i, e, _, bound in chunks] == [(512, "in"), (512, "in"), (6, "end")]
    assert b.total == 8 * n and (b.status & dm.L4_CSUM_SET).all()
    b.check_host()


# ---- 8. unchanged behaviour ----
def test_launch_names_and_the_plain_framer_in_the_same_process(dev, oracle, inet_oracle):
    rng = np.random.default_rng(513)
    dgs = [l4_datagram(rng, PROTOS[q % 3], HLENS[q % 3], L) for q, L in enumerate((0, 30, 999, 1480, 3000, 10000))]
    for flags, name, plain in ((FCS, "general-l4-fcs", "general-fcs"), (0, "general-l4", "general")):
        b = DBatch(oracle, inet_oracle, dgs, 1500, flags, seed=44)
        out_f, st_f = b.run_txf_dev(dev)
        assert na.txf_last_launch() == plain
        b.check_dev(b.run_dev(dev))
        assert na.txd_last_launch() == name and na.txf_last_launch() == plain
        out_f2, st_f2 = b.run_txf_dev(dev)
        assert np.array_equal(out_f, b.txf_expect) and np.array_equal(out_f2, b.txf_expect)
        assert np.array_equal(st_f, b.txf_status) and np.array_equal(st_f2, b.txf_status)
        assert not np.array_equal(b.txf_expect, b.expect)


# ---- 9. no fallback ----
def test_host_counters_stay_untouched(dev, oracle, inet_oracle):
    L = na.load()
    before = (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks())
    rng = np.random.default_rng(514)
    b = DBatch(oracle, inet_oracle, [l4_datagram(rng, 17, 20, 5000), l4_datagram(rng, 6, 24, 100)], 1500, FCS, seed=45)
    b.check(dev)
    assert (L.fcs_engine_host_batches(), L.fcs_engine_host_fallbacks()) == before
