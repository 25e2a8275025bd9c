"""CPU tests of the frame generator tests/rxv_traffic.py: every frame of the sweeps that
tests/test_gpu_rxv_cuts.py sends through the kernels gets the verdict it was built for from the
model (tests/rxv_model.py, the oracle's arithmetic) and from the independent witness
(make_rxv_golden.expect), no requested cut is missing, and the mixed fixed-length traffic reaches
every verdict class in every quarter of an LDS-DMA item. Conditions on the inputs, no tolerances."""
import numpy as np
import pytest

import rxv_model as rm
import rxv_traffic as rt

gen = rt.gen


def check_sweep(oracle, inet_oracle, sw, trailer):
    flags = rm.F_TRAILER if trailer else 0
    bad = []
    for fr, want, info in zip(sw.frames, sw.expect, sw.info):
        m, e = rm.verdict(oracle, inet_oracle, fr, flags), gen.expect(fr, flags)
        if not (m == e == int(want)):
            bad.append((info, hex(m), hex(e), hex(int(want))))
    assert not bad, (len(bad), bad[:8])
    # the other flag value has no constructed verdict (the trailer is then payload, or missing): the
    # model and the witness still agree
    other = flags ^ rm.F_TRAILER
    bad = [sw.info[i] for i in range(len(sw))
           if rm.verdict(oracle, inet_oracle, sw.frames[i], other) != gen.expect(sw.frames[i], other)]
    assert not bad, (len(bad), bad[:8])


def check_witnesses(sw, F, trailer):
    """Each cut comes with its clean frame, the bent last byte and (with padding) the bent byte behind."""
    T = 4 if trailer else 0
    assert all(len(fr) == F for fr in sw.frames)
    by = {}
    for i, (kind, hlen, cl, which) in enumerate(sw.info):
        assert which not in by.setdefault((kind, hlen, cl), {})
        by[(kind, hlen, cl)][which] = i
    for (kind, hlen, cl), d in by.items():
        assert set(d) == ({"clean", "last", "behind"} if cl < F - T else {"clean", "last"}), (kind, hlen, cl)
    M = sw.matrix()
    cols = np.arange(F)
    for which, shift in (("last", -1), ("behind", 0)):
        keys = [k for k, d in by.items() if which in d]
        diff = M[[by[k]["clean"] for k in keys]] != M[[by[k][which] for k in keys]]
        pos = np.array([k[2] + shift for k in keys])
        assert np.array_equal(diff, cols[None, :] == pos[:, None]), which   # exactly that byte differs
    keys = list(by)
    cl = np.array([k[2] for k in keys])
    behind = (cols[None, :] >= cl[:, None]) & (cols[None, :] < F - T)
    assert not np.any((M[[by[k]["clean"] for k in keys]] == 0) & behind)   # nothing behind the datagram is zero


@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", sorted(set(rt.DMA_LENGTHS + rt.FULL_LENGTHS)))
def test_full_sweeps(oracle, inet_oracle, F, trailer):
    sw = rt.full_sweep(F, trailer)
    T = 4 if trailer else 0
    want = {(kind, hlen, cl) for kind in rt.KINDS for hlen in rt.SWEEP_HLENS
            for cl in range(14 + hlen + rt.L4HDR[kind], F - T + 1)}
    assert rt.cut_positions(sw) == want
    if F > 1000:
        assert 8000 <= len(want) <= 9000 and len(sw) > 25000
    else:
        assert len(want) >= 4   # 60 bytes: only hlen 20 fits
    check_witnesses(sw, F, trailer)
    check_sweep(oracle, inet_oracle, sw, trailer)


@pytest.mark.parametrize("kind", rt.KINDS)
@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", rt.SEG_LENGTHS)
def test_segment_sweeps(oracle, inet_oracle, F, trailer, kind):
    sw = rt.seg_sweep(F, trailer, kind)
    T = 4 if trailer else 0
    cuts = rt.segment_cuts(F, seed=F)
    for k in range(F // 1536 + 1):      # the borders themselves, both sides
        assert {F - 1536 * k - 100, F - 1536 * k - 1, F - 1536 * k, F - 1536 * k + 1} & set(range(F + 1)) <= cuts
    for j in range(4):
        assert {F - 96 * j - 100, F - 96 * j, min(F - 96 * j + 100, F)} <= cuts
    want = {(kind, hlen, cl) for hlen in rt.SWEEP_HLENS for cl in cuts if 14 + hlen + rt.L4HDR[kind] <= cl <= F - T}
    assert rt.cut_positions(sw) == want
    assert len({cl for _, _, cl in want}) >= 500
    check_witnesses(sw, F, trailer)
    check_sweep(oracle, inet_oracle, sw, trailer)


@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", [1518, 1600])
def test_quirk_frames(oracle, inet_oracle, F, trailer):
    sw = rt.quirk_frames(F, trailer)
    assert len(sw) == 2 * (3 * 5 + 1)
    T = 4 if trailer else 0
    for (kind, hlen, cl, which), fr in zip(sw.info, sw.frames):
        fill = int(which[-2:], 16)
        assert set(fr[cl:F - T]) == {fill}
        if which.startswith("zeros"):
            assert fr[34:42] == bytes(8)
    check_sweep(oracle, inet_oracle, sw, trailer)


@pytest.mark.parametrize("trailer", [True, False])
def test_variable_mix(oracle, inet_oracle, trailer):
    sw = rt.variable_mix(6000, trailer, seed=31 + trailer)
    lens = np.array([len(f) for f in sw.frames])
    assert lens.min() >= 60 and lens.max() <= 9018 and 150 <= np.count_nonzero(lens > 1536) <= 450
    assert {h for _, h, _, _ in sw.info} == set(rt.HLENS)
    assert {k for k, _, _, _ in sw.info} == set(rt.KINDS)
    assert np.count_nonzero(sw.expect & rm.IP_BAD_LEN) > 5000   # nearly every frame has bytes behind the datagram
    check_sweep(oracle, inet_oracle, sw, trailer)


@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", [1496, 1518, 1524, 97])
def test_mixed_fixed_reaches_every_class(oracle, inet_oracle, F, trailer):
    flags = rm.F_TRAILER if trailer else 0
    frames = rt.mixed_fixed(F, 1000, trailer, seed=F)
    assert len(frames) == 1000 and all(len(f) == F for f in frames)
    assert frames == rt.mixed_fixed(F, 1000, trailer, seed=F)   # deterministic
    v = np.array([rm.verdict(oracle, inet_oracle, f, flags) for f in frames], dtype=np.uint32)
    assert np.array_equal(v, np.array([gen.expect(f, flags) for f in frames], dtype=np.uint32))
    # every bit a frame of this length can get (RUNT needs F < 14 + T; FCS_BAD the trailer flag)
    bits = [rm.IPV4, rm.IP_BAD_HDR, rm.IP_BAD_LEN, rm.IP_BAD_CSUM, rm.FRAG, rm.L4_CHECKED, rm.L4_BAD_CSUM, rm.L4_SHORT]
    for bit in bits + ([rm.FCS_BAD] if trailer else []):
        assert np.count_nonzero(v & np.uint32(bit)) >= 10, hex(bit)
    assert np.count_nonzero((v & rm.IPV4) == 0) >= 10                      # other ethertypes
    assert np.count_nonzero(v == (rm.IPV4 | (17 << 16))) >= 10             # UDP, no checksum sent
    clean = [np.uint32(rt.clean_verdict(k, 0)) for k in rt.KINDS]
    assert all(np.count_nonzero(v == c) >= 10 for c in clean)
    hl = {(f[14] & 15) * 4 for f, w in zip(frames, v) if w & rm.L4_CHECKED and not w & rm.L4_BAD_CSUM}
    if F > 200:   # at 97 bytes the long headers leave no room for a TCP header
        assert hl == set(rt.HLENS), hl
    for g in range(4):
        for proto in (1, 6, 17):
            q = v[g::4]
            assert np.count_nonzero(((q >> 16) & 0xFF == proto) & ((q & rm.L4_CHECKED) != 0)) >= 3, (g, proto)
        for bit in bits:
            assert np.count_nonzero(v[g::4] & np.uint32(bit)), (g, hex(bit))


def test_tiny_fixed():
    for F in (0, 3, 17, 18, 37):
        fr = rt.tiny_fixed(F, 33, seed=F)
        assert len(fr) == 33 and all(len(f) == F for f in fr)
