"""GPU tests of one-pass TX framing at the borders its walk has: frames whose length is a multiple
of the 1536-byte segment (lane 15 starts at frame position 0 and the word carried from the frame
before is stale), first segments shorter than the header image, the largest mtu (43 segments),
datagram arenas exactly as large as the datagram at every pointer alignment, and header checksums
of 0x0000. Method as in tests/test_gpu_txf.py: the whole canaried output arena, flen, fcs, status,
first and the plan's status against the model, device form after the plan call and host form."""
import numpy as np
import pytest

import nstack_amd as na
import txf_model as fm
from txf_batch import FCS, Batch, datagram

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SEG = 1536   # fcs::kSegBytes: a quarter-wave pass


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def frame_at(b, k):
    """Frame bytes (without the FCS) of slot k in the model's arena."""
    o = b.base + k * b.slot
    return b.expect[o:o + int(b.flen[k])]


# ---- D: frames of 1536 k + t bytes ----
def multiples(rng, ks, more=()):
    """Whole datagrams whose frames are 1536 k + t bytes, t = -4..4, each behind a short frame of random
    bytes; `more`: further (hlen, D). Returns the datagrams and the indices and F of the targets."""
    dgs, at = [], []
    for k in ks:
        for t in range(-4, 5):
            F = SEG * k + t
            hlen = (20, 60, 24)[(t + 4) % 3]
            dgs.append(datagram(rng, 20, int(rng.integers(60, 1400))))
            at.append((len(dgs), F))
            dgs.append(datagram(rng, hlen, F - 14 - hlen))
    for hlen, D in more:
        dgs.append(datagram(rng, 20, int(rng.integers(60, 1400))))
        at.append((len(dgs), D + 14))
        dgs.append(datagram(rng, hlen, D - hlen))
    return dgs, at


def check_multiples(dev, oracle, inet_oracle, dgs, at, mtu, flags, base, want_mod):
    for extra in (0, 1):
        b = Batch(oracle, inet_oracle, dgs, mtu, flags, slot=fm.min_slot(mtu, flags) + extra, base=base, seed=mtu + base)
        assert (b.status == fm.WHOLE).all() and b.total == b.n
        assert {F % SEG for _, F in at} >= want_mod
        for i, F in at:
            assert b.flen[i] == F
            assert frame_at(b, i - 1)[-4:].any()      # the word carried over from the frame in front is not zero
            assert i % 8                              # ... and that frame is the same row's (same run of eight)
        b.check(dev, host=base in (0, 3))


NEAR = set(range(0, 5)) | set(range(SEG - 4, SEG))


@pytest.mark.parametrize("base", [0, 1, 2, 3])
@pytest.mark.parametrize("flags", [FCS, 0])
def test_frames_of_whole_segments(dev, oracle, inet_oracle, flags, base):
    """F = 1536 k + t for k = 1, 2, 3 and t = -4..4: at t = 0 lane 15 of the first segment starts at frame
    position 0, at t = 1..4 the first segment is one to four bytes."""
    dgs, at = multiples(np.random.default_rng(21), (1, 2, 3))
    assert {F // SEG for _, F in at if F % SEG == 0} == {1, 2, 3}
    check_multiples(dev, oracle, inet_oracle, dgs, at, 4800, flags, base, NEAR)


@pytest.mark.parametrize("base", [0, 1, 2, 3])
@pytest.mark.parametrize("flags", [FCS, 0])
def test_largest_mtu(dev, oracle, inet_oracle, flags, base):
    """mtu 65535: F = 1536 * 42 + t, and the largest frames there are (65535 bytes with a 20- and a
    60-byte header, 65534 bytes): 43 segments of the CRC and carry chain."""
    dgs, at = multiples(np.random.default_rng(22), (42,), more=((20, 65535), (60, 65535), (24, 65534)))
    assert max(F for _, F in at) == 65549 and -(-65549 // SEG) == 43
    check_multiples(dev, oracle, inet_oracle, dgs, at, 65535, flags, base, NEAR)


# ---- D: first segments of 1..80 bytes (the header image is 34 to 74 bytes) ----
@pytest.mark.parametrize("flags", [FCS, 0])
def test_short_first_segments(dev, oracle, inet_oracle, flags):
    mtu, rng = 1700, np.random.default_rng(23)
    whole = [datagram(rng, hlen, 1522 + t - hlen) for hlen in (20, 60) for t in range(1, 81)]
    mx = fm.frag_unit(mtu, 60)
    assert mx == 1632
    frag = [datagram(rng, 60, mx + 1536 + t - 74) for t in range(1, 81)]
    for base, extra in ((0, 0), (1, 1), (2, 0), (3, 1)):
        b = Batch(oracle, inet_oracle, whole + frag, mtu, flags, slot=fm.min_slot(mtu, flags) + extra, base=base, seed=31)
        nw = len(whole)
        assert (b.status[:nw] == fm.WHOLE).all() and (b.status[nw:] == fm.FRAGMENTED).all()
        assert b.total == nw + 2 * len(frag)
        # the first segment of a frame is what is left in front of whole segments counted from its end
        for part in (b.flen[:80], b.flen[80:160], b.flen[nw + 1:b.total:2]):
            assert sorted(int(F) - SEG for F in part) == list(range(1, 81))
        assert (b.flen[nw:b.total:2] == 14 + 60 + mx).all()
        b.check(dev, host=extra == 0)


# ---- E: arenas exactly as large as the datagram ----
EDGE_D = [20, 21, 23, 59, 60, 61, 95, 96, 97, 110, 111, 1500, 1501, 3000]


def tight(oracle, inet_oracle, rng, hlen, D, mtu, r):
    dg = datagram(rng, hlen, D - hlen)
    return Batch(oracle, inet_oracle, None, mtu, FCS, placed=(np.frombuffer(dg, dtype=np.uint8), [0], [D]),
                 slot=fm.min_slot(mtu, FCS) + 1, base=r, seed=D + r, front=r, back=9)


@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_arena_exactly_the_datagram(dev, oracle, inet_oracle, r):
    """One datagram, dgram = an aligned base + r, dgram_bytes = its length: every load in front of it
    and behind it is refused or masked (random bytes lie on both sides inside the same dwords). The
    plan call runs on the same arena; its status and first[] are compared too. One synchronise for
    the launches of an alignment."""
    rng = np.random.default_rng(40 + r)
    bs = [tight(oracle, inet_oracle, rng, hlen, D, 1500, r) for D in EDGE_D for hlen in sorted({20, min(60, D & ~3)})]
    bs += [tight(oracle, inet_oracle, rng, hlen, 3000, 76, r) for hlen in (20, 60)]
    assert [b.total for b in bs[-2:]] == [63, 368]
    assert {int(s) for b in bs for s in b.status} == {fm.WHOLE, fm.FRAGMENTED}
    for b in bs:
        assert b.around.size == r + b.arena.size + 9 and b.arena.size == int(b.ln[0])
    launched = [b.launch_dev(dev) for b in bs]
    torch.cuda.synchronize()
    for b, t in zip(bs, launched):
        b.check_dev(b.collect(t))
    for b in bs[::7]:
        b.check_host()


@pytest.mark.parametrize("r", [0, 1, 2, 3])
def test_descending_offsets_flush_with_both_ends(dev, oracle, inet_oracle, r):
    """Three datagrams, off[] descending: datagram 0 ends with the arena, datagram 2 begins it."""
    rng = np.random.default_rng(50 + r)
    dgs = [datagram(rng, 24, 3000 - 24), datagram(rng, 20, 41), datagram(rng, 60, 1501 - 60)]
    gap = [rng.integers(0, 256, g, dtype=np.uint8) for g in (5 - r, 2 + r)]
    arena = np.concatenate([np.frombuffer(dgs[2], dtype=np.uint8), gap[0], np.frombuffer(dgs[1], dtype=np.uint8), gap[1],
                            np.frombuffer(dgs[0], dtype=np.uint8)])
    off = [arena.size - 3000, 1501 + gap[0].size, 0]
    assert off[0] > off[1] > off[2] == 0 and off[0] + 3000 == arena.size
    for mtu in (1500, 76):
        b = Batch(oracle, inet_oracle, None, mtu, FCS, placed=(arena, off, [3000, 61, 1501]), base=r, seed=60 + r,
                  front=r, back=7)
        assert b.total == (3 + 1 + 2 if mtu == 1500 else 62 + 1 + 181)
        b.check(dev)


# ---- F: header checksums of 0x0000 ----
def zero_checksum(oracle, inet_oracle, dg, mtu, j):
    """dg with the id that makes the header checksum of its frame j 0x0000: the one's-complement sum
    of the other words is ~c for the checksum c at id = 0, so id = c folds the sum to 0xFFFF."""
    d = bytearray(dg)
    d[4:6] = b"\x00\x00"
    c = fm.frames(oracle, inet_oracle, bytes(d), bytes(12), mtu, 0)[1][j][24:26]
    d[4:6] = c
    return bytes(d)


@pytest.mark.parametrize("flags", [FCS, 0])
def test_header_checksum_zero(dev, oracle, inet_oracle, flags):
    mtu, rng = 576, np.random.default_rng(70)
    dgs, at = [], []
    for hlen in (20, 60):
        mx = fm.frag_unit(mtu, hlen)
        for B, j in ((300, 0), (3 * mx + 77, 0), (3 * mx + 77, 2), (3 * mx + 77, 3)):
            dgs.append(datagram(rng, 20, int(rng.integers(0, 2000))))
            at.append((len(dgs), j))
            dgs.append(zero_checksum(oracle, inet_oracle, datagram(rng, hlen, B), mtu, j))
    for base, extra in ((0, 0), (3, 1)):
        b = Batch(oracle, inet_oracle, dgs, mtu, flags, slot=fm.min_slot(mtu, flags) + extra, base=base, seed=71)
        zeros = 0
        for i, j in at:
            cnt = int(b.plan_first[i + 1] - b.plan_first[i])
            assert cnt == (1 if j == 0 and b.status[i] == fm.WHOLE else 4)
            for q in range(cnt):
                csum = frame_at(b, int(b.plan_first[i]) + q)[24:26].tobytes()
                assert (csum == b"\x00\x00") == (q == j), (i, q)
                zeros += q == j
        assert zeros == 8
        b.check(dev)
