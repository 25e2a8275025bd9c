"""GPU tests of one-pass TX sealing (include/nstack_txs.h) through the C ABI: the device, fixed and
host forms must leave byte-identical arenas, status words and fields records, equal to the model's
(tests/txs_model.py: the header's rules with the oracle's CRC and checksums) and to the
independently generated golden vectors. Every frame sits between canary bytes and the whole arena
is compared, so a write to any other byte fails the test."""
import json
import os
import socket
import threading

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm
import txs_model as tm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FLAGS = (tm.F_FCS, 0, tm.F_FCS | tm.F_UDP_ZERO)
PROTOS = (6, 17, 1)
L4MIN = {6: 20, 17: 8, 1: 4}
HLENS = tuple(range(20, 64, 4))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def txs_golden():
    with open(os.path.join(GOLDEN, "txs_vectors.json")) as f:
        vec = json.load(f)
    with open(os.path.join(GOLDEN, vec["input"]), "rb") as f:
        vec["input_bytes"] = f.read()
    vec["sealed_bytes"] = []
    for name in vec["sealed"]:
        with open(os.path.join(GOLDEN, name), "rb") as f:
            vec["sealed_bytes"].append(f.read())
    return vec


@pytest.fixture(params=["general", "dma"], autouse=True)
def txs_kernel(request):
    """Every test runs under both DMA thresholds (identical bytes required): general = 1 << 63, a
    quarter-wave per frame with register loads for every batch; dma = 0, fixed-stride batches whose
    geometry fits the LDS-DMA kernel's slots through txs_dma_kernel. Variable and host batches always
    take the general kernel (txs::route)."""
    old = na.tx_seal_set_dma_threshold(0 if request.param == "dma" else (1 << 63))
    yield request.param
    na.tx_seal_set_dma_threshold(old)


_REF = {}   # model results, computed once per batch and shared by both kernel parameters


def reference(key, oracle, inet_oracle, arena, off, ln, flags):
    k = (key, flags)
    if k not in _REF:
        out, st, fl = tm.seal_arena(oracle, inet_oracle, arena, off, ln, flags)
        out.setflags(write=False)
        st.setflags(write=False)
        fl.setflags(write=False)
        _REF[k] = (out, st, fl)
    return _REF[k]


def to_dev(arr, dev):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def raw_frame(rng, F, hlen, proto, pad=0, df=True):
    """F random bytes with an IPv4 header stamped on: every checksum field is garbage."""
    b = bytearray(rng.integers(0, 256, F, dtype=np.uint8).tobytes())
    b[12:14] = b"\x08\x00"
    b[14] = 0x40 | (hlen // 4)
    b[16:18] = int(F - 14 - pad).to_bytes(2, "big")
    b[20:22] = b"\x40\x00" if df else b"\x00\x00"
    b[23] = proto
    return bytes(b)


def pack(frames, aligns=None, seed=1, gap=(0, 12), mod=16):
    """Frames into one arena of canary (random) bytes: frame i starts at aligns[i] mod `mod`, four
    bytes of FCS place and a canary gap behind it."""
    rng = np.random.default_rng(seed)
    total = sum(len(f) + 4 + gap[1] + mod for f in frames) + 64
    arena = rng.integers(0, 256, total, dtype=np.uint8)
    off, pos = [], 0
    for i, fr in enumerate(frames):
        a = int(rng.integers(0, mod)) if aligns is None else aligns[i]
        pos += (a - pos) % mod
        off.append(pos)
        arena[pos:pos + len(fr)] = np.frombuffer(fr, dtype=np.uint8)
        pos += len(fr) + 4 + int(rng.integers(gap[0], gap[1] + 1))
    return arena[:pos + 16].copy(), np.array(off, dtype=np.uint64), np.array([len(f) for f in frames], dtype=np.uint32)


def run_dev(dev, arena, off, ln, flags, count_mask=0, status=True, fields=True, count=True, stream=None):
    """(arena after, status, fields, count) of the variable device form."""
    n = len(off)
    d_arena = to_dev(arena, dev)
    d_off = to_dev(np.asarray(off, dtype=np.uint64).view(np.int64), dev)
    d_len = to_dev(np.asarray(ln, dtype=np.uint32).view(np.int32), dev)
    st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev) if status else None
    fl = torch.full((max(n, 1), 2), -1, dtype=torch.int32, device=dev) if fields else None
    cnt = torch.full((1,), 77, dtype=torch.int64, device=dev) if count else None
    na.tx_seal_dev(d_arena, arena.nbytes, d_off, d_len, n, flags=flags, count_mask=count_mask, status=st, fields=fl,
                   count=cnt, stream=stream)
    torch.cuda.synchronize()
    if n:   # variable batches always take the general kernel
        assert na.txs_last_launch() == "general"
    return (d_arena.cpu().numpy(), st.cpu().numpy().view(np.uint32)[:n] if status else None,
            fl.cpu().numpy().view(tm.FIELDS_DTYPE).reshape(-1)[:n] if fields else None,
            int(cnt.item()) if count else None)


def run_fixed(dev, arena, base, stride, length, n, flags, count_mask=0):
    d_arena = to_dev(arena, dev)
    st = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    fl = torch.full((max(n, 1), 2), -1, dtype=torch.int32, device=dev)
    cnt = torch.full((1,), 5, dtype=torch.int64, device=dev)
    na.tx_seal_fixed_dev(d_arena.data_ptr() + base, stride, length, n, flags=flags, count_mask=count_mask, status=st,
                         fields=fl, count=cnt)
    torch.cuda.synchronize()
    return (d_arena.cpu().numpy(), st.cpu().numpy().view(np.uint32)[:n],
            fl.cpu().numpy().view(tm.FIELDS_DTYPE).reshape(-1)[:n], int(cnt.item()), d_arena.data_ptr() + base)


def run_host(arena, off, ln, flags, count_mask=0):
    a = arena.copy()
    st = np.full(len(off), 0xDEADBEEF, dtype=np.uint32)
    cnt = na.tx_seal_host(a, a.nbytes, off, ln, len(off), flags=flags, count_mask=count_mask, status=st)
    if len(off):   # the host form's chunks are variable batches: the general kernel
        assert na.txs_last_launch() == "general"
    return a, st, cnt


def assert_same(got, exp, what, info=None, off=None, ln=None):
    g, e = np.asarray(got), np.asarray(exp)
    assert g.shape == e.shape, (what, g.shape, e.shape)
    bad = np.nonzero(g != e)[0]
    if bad.size and off is not None:   # arena bytes: name the frames the first differing bytes belong to
        who = [(int(p), int(np.searchsorted(off, p, side="right")) - 1) for p in bad[:6]]
        detail = [(p, i, p - int(off[i]), int(ln[i]), info[i] if info else None, int(g[p]), int(e[p])) for p, i in who]
        raise AssertionError((what, "bytes differ", int(bad.size), detail))
    assert bad.size == 0, (what, int(bad.size), [(int(i), g[i], e[i], info[i] if info else None) for i in bad[:8]])


def check_all_forms(dev, oracle, inet_oracle, key, arena, off, ln, flags, info=None, fixed=None, count_mask=None):
    """Device, host and (fixed = (base, stride, length)) fixed forms against the model."""
    exp_a, exp_s, exp_f = reference(key, oracle, inet_oracle, arena, off, ln, flags)
    mask = tm.L4_CSUM_SET | tm.RUNT if count_mask is None else count_mask
    want = int(np.count_nonzero(exp_s & np.uint32(mask)))
    a, s, f, c = run_dev(dev, arena, off, ln, flags, mask)
    assert na.txs_last_launch() == "general"
    assert_same(s, exp_s, (key, flags, "dev status"), info)
    assert_same(f, exp_f, (key, flags, "dev fields"), info)
    assert_same(a, exp_a, (key, flags, "dev arena"), info, off, ln)
    assert c == want
    a, s, c = run_host(arena, off, ln, flags, mask)
    assert_same(s, exp_s, (key, flags, "host status"), info)
    assert_same(a, exp_a, (key, flags, "host arena"), info, off, ln)
    assert c == want
    if fixed is not None:
        base, stride, length = fixed
        a, s, f, c, ptr = run_fixed(dev, arena, base, stride, length, len(off), flags, mask)
        assert na.txs_last_launch() == na.txs_route(ptr, stride, length, len(off), flags)
        assert_same(s, exp_s, (key, flags, "fixed status"), info)
        assert_same(f, exp_f, (key, flags, "fixed fields"), info)
        assert_same(a, exp_a, (key, flags, "fixed arena"), info, off, ln)
        assert c == want
        return na.txs_last_launch()
    return "general"


# ---- 1. golden vectors, each at the start alignments 0..3 ----
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_golden_vectors(dev, txs_golden, flags):
    recs = txs_golden["frames"]
    a = txs_golden["input_bytes"]
    arena = np.frombuffer(a, dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    tags = [r["tag"] for r in recs]
    exp_s = np.array([r["status"][flags] for r in recs], dtype=np.uint32)
    exp_f = np.array([tuple(r["fields"][flags]) for r in recs], dtype=tm.FIELDS_DTYPE)
    exp_a = np.frombuffer(txs_golden["sealed_bytes"][flags], dtype=np.uint8)
    got_a, s, f, _ = run_dev(dev, arena, off, ln, flags)
    assert_same(s, exp_s, "golden status", tags)
    assert_same(f, exp_f, "golden fields", tags)
    assert_same(got_a, exp_a, "golden arena", tags, off, ln)
    got_a, s, _ = run_host(arena, off, ln, flags)
    assert_same(s, exp_s, "golden host status", tags)
    assert_same(got_a, exp_a, "golden host arena", tags, off, ln)
    # repacked: every frame at the start alignments 0..3 (mod 4), the golden sealed bytes expected
    for al in range(4):
        frames = [a[r["off"]:r["off"] + r["len"] + 4] for r in recs]   # with the garbage FCS place
        ar2, off2, _ = pack([fr[:-4] for fr in frames], [al] * len(frames), seed=al, gap=(4, 4), mod=4)
        exp2 = ar2.copy()
        for r, o in zip(recs, off2):
            n_out = r["len"] + (4 if flags & tm.F_FCS else 0)
            exp2[int(o):int(o) + n_out] = exp_a[r["off"]:r["off"] + n_out]
        got, s, f, _ = run_dev(dev, ar2, off2, ln, flags)
        assert_same(s, exp_s, ("golden status", al), tags)
        assert_same(f, exp_f, ("golden fields", al), tags)
        assert_same(got, exp2, ("golden arena", al), tags, off2, ln)


# ---- 2. straddle sweep, general kernel: every residue of F mod 96 for every field position ----
def straddle_batch():
    rng = np.random.default_rng(2024)
    frames, info = [], []
    for F in range(130, 331):
        for hlen in HLENS:
            for proto in PROTOS:
                room = F - 14 - hlen - L4MIN[proto]
                if room < 0:
                    continue
                pad = int(rng.integers(0, min(room, 40) + 1)) if rng.random() < 0.5 else 0
                frames.append(raw_frame(rng, F, hlen, proto, pad))
                info.append((F, hlen, proto, pad))
    return frames, info


def test_straddle_sweep(dev, oracle, inet_oracle):
    frames, info = straddle_batch()
    assert len(frames) > 6000
    arena, off, ln = pack(frames, seed=5)
    for flags in FLAGS:
        check_all_forms(dev, oracle, inet_oracle, "straddle", arena, off, ln, flags, info)
    # second pass: the fields zeroed beforehand must give identical output
    zeroed = arena.copy()
    for o, (F, hlen, proto, _) in zip(off, info):
        o = int(o)
        zeroed[o + 24:o + 26] = 0
        q = o + 14 + hlen + tm.L4_FIELD[proto]
        zeroed[q:q + 2] = 0
    exp_a, exp_s, exp_f = reference("straddle", oracle, inet_oracle, arena, off, ln, tm.F_FCS)
    a, s, f, _ = run_dev(dev, zeroed, off, ln, tm.F_FCS)
    assert_same(s, exp_s, "zeroed status", info)
    assert_same(f, exp_f, "zeroed fields", info)
    assert_same(a, exp_a, "zeroed arena", info, off, ln)


# ---- 3. segment borders ----
def border_batch():
    rng = np.random.default_rng(77)
    frames, info = [], []
    for F in range(1537, 1741):
        for hlen in (20, 44, 60):
            for proto in PROTOS:
                pad = int(rng.integers(0, 30)) if rng.random() < 0.3 else 0
                frames.append(raw_frame(rng, F, hlen, proto, pad))
                info.append((F, hlen, proto, pad))
    for F in range(3073, 3271):
        for hlen in (20, 60):
            frames.append(raw_frame(rng, F, hlen, 6))
            info.append((F, hlen, 6, 0))
    for F, hlen, proto in ((9018, 20, 6), (9018, 60, 17), (9018, 36, 1), (65535, 20, 6), (65535, 60, 17), (65535, 24, 1)):
        frames.append(raw_frame(rng, F, hlen, proto))
        info.append((F, hlen, proto, 0))
    return frames, info


def test_segment_borders_variable(dev, oracle, inet_oracle):
    frames, info = border_batch()
    arena, off, ln = pack(frames, seed=6)
    for flags in FLAGS:
        check_all_forms(dev, oracle, inet_oracle, "borders", arena, off, ln, flags, info)


@pytest.mark.parametrize("F", [1537, 1538, 1561, 1562, 1627, 1628, 1633, 3073, 3097, 3163, 9018, 65535])
def test_segment_borders_fixed(dev, oracle, inet_oracle, F):
    rng = np.random.default_rng(F)
    n = 7 if F > 9018 else 37
    for base, stride in ((0, F + 4), (1, F + 5), (3, F + 11)):
        arena = rng.integers(0, 256, base + n * stride + 8, dtype=np.uint8)
        info = []
        for i in range(n):
            hlen, proto = HLENS[(i + base) % 11], PROTOS[i % 3]
            fr = raw_frame(rng, F, hlen, proto, pad=(i % 5) * 3)
            arena[base + i * stride:base + i * stride + F] = np.frombuffer(fr, dtype=np.uint8)
            info.append((hlen, proto))
        off = base + np.arange(n, dtype=np.uint64) * stride
        ln = np.full(n, F, dtype=np.uint32)
        for flags in (tm.F_FCS, 0):
            assert check_all_forms(dev, oracle, inet_oracle, ("fixed", F, base), arena, off, ln, flags, info,
                                   fixed=(base, stride, F)) == "general"


def fixed_batch_check(dev, oracle, inet_oracle, key, F, combos, flags_list=(tm.F_FCS, 0)):
    """One fixed-stride batch of len(combos) frames of F bytes, frame i with combos[i] = (hlen,
    protocol); start alignment and stride vary with F. The fixed form against the model."""
    rng = np.random.default_rng(F * 31 + len(combos))
    n, base, stride = len(combos), F % 4, F + 4 + F % 7
    arena = rng.integers(0, 256, base + (n - 1) * stride + F + 4, dtype=np.uint8)   # ends with the last FCS place
    for i, (hlen, proto) in enumerate(combos):
        room = F - 14 - hlen - L4MIN[proto]
        fr = raw_frame(rng, F, hlen, proto, pad=min(room, (i % 4) * 5))
        arena[base + i * stride:base + i * stride + F] = np.frombuffer(fr, dtype=np.uint8)
    off = base + np.arange(n, dtype=np.uint64) * stride
    ln = np.full(n, F, dtype=np.uint32)
    for flags in flags_list:
        exp_a, exp_s, exp_f = reference(key, oracle, inet_oracle, arena, off, ln, flags)
        a, s, f, c, ptr = run_fixed(dev, arena, base, stride, F, n, flags, tm.L4_CSUM_SET)
        assert na.txs_last_launch() == na.txs_route(ptr, stride, F, n, flags) == "general"
        assert_same(s, exp_s, (key, flags, "fixed status"), combos)
        assert_same(f, exp_f, (key, flags, "fixed fields"), combos)
        assert_same(a, exp_a, (key, flags, "fixed arena"), combos, off, ln)
        assert c == int(np.count_nonzero(exp_s & np.uint32(tm.L4_CSUM_SET)))


@pytest.mark.parametrize("lo", [1537, 1588, 1639, 1690])
def test_segment_borders_fixed_every_length_two_segments(dev, oracle, inet_oracle, lo):
    """Every F in 1537..1740, header lengths 20, 44 and 60, three protocols, through the fixed form
    (front segments of 1..204 bytes: every residue of F mod 96, the fields in segment 1 or astride)."""
    for F in range(lo, min(lo + 51, 1741)):
        fixed_batch_check(dev, oracle, inet_oracle, ("fixed2", F), F, [(h, p) for h in (20, 44, 60) for p in PROTOS])


@pytest.mark.parametrize("lo", [3073, 3172])
def test_segment_borders_fixed_every_length_three_segments(dev, oracle, inet_oracle, lo):
    """Every F in 3073..3270, TCP, header lengths 20 and 60, through the fixed form."""
    for F in range(lo, min(lo + 99, 3271)):
        fixed_batch_check(dev, oracle, inet_oracle, ("fixed3", F), F, [(20, 6), (60, 6), (60, 6), (20, 6), (20, 6)])


@pytest.mark.parametrize("F", [2977, 2998, 3024, 3071, 3072, 4513, 4608])
def test_fixed_multi_segment_frames_with_a_short_front_mask(dev, oracle, inet_oracle, F):
    """Fixed multi-segment lengths whose front segment holds 1441..1536 bytes: the front-mask loop runs
    with a bound below a whole chunk (the single-segment band lengths are the only other such shapes)."""
    assert 1441 <= (F - 1) % 1536 + 1 <= 1536 and F > 1536
    fixed_batch_check(dev, oracle, inet_oracle, ("fixedz", F), F, [(h, p) for h in HLENS for p in PROTOS][::2])


@pytest.mark.parametrize("lo", [130, 231])
def test_straddle_sweep_fixed(dev, oracle, inet_oracle, lo):
    """The straddle sweep through the fixed form: every F in 130..330, all eleven header lengths and
    the three protocols where the segment fits."""
    for F in range(lo, min(lo + 101, 331)):
        combos = [(h, p) for h in HLENS for p in PROTOS if F - 14 - h - L4MIN[p] >= 0]
        assert len(combos) == 33
        fixed_batch_check(dev, oracle, inet_oracle, ("fixeds", F), F, combos, flags_list=(tm.F_FCS,))


# ---- 4. the LDS-DMA band: 29 lengths x 5 strides x 16 start alignments, batches of 9..12, 70 and 259 ----
def band_cases(F):
    """(stride, start alignment, frames): five strides from F + 4 to the widest in-band one, each at
    all 16 start alignments; batches of 9..12 frames (every slot clamped to the arena's end), and one
    of 70 and one of 259 per stride (last items of 2 and 3 frames; 9..12 give 1..4)."""
    wide = min(2048, (6126 - F) // 3)
    cases = []
    for si, stride in enumerate((F + 4, F + 5, min(F + 16, wide), (F + 4 + wide) // 2, wide)):
        for align in range(16):
            n = 70 if align == (3 + si) % 16 else (259 if align == (9 + si) % 16 else 9 + (align + si) % 4)
            cases.append((stride, align, n))
    return cases


@pytest.mark.parametrize("F", list(range(1496, 1525)))
def test_lds_dma_band(dev, oracle, inet_oracle, txs_kernel, F):
    seen = set()
    for stride, align, n in band_cases(F):
        rng = np.random.default_rng(F * 4099 + stride * 17 + align)
        # the arena ends with the last frame's FCS place: the last items' slots are clamped to its end
        size = align + (n - 1) * stride + F + 4
        arena = rng.integers(0, 256, size, dtype=np.uint8)
        info = []
        for i in range(n):
            hlen, proto = HLENS[(i + stride + align) % 11], PROTOS[(i // 11 + i + align) % 3]
            fr = raw_frame(rng, F, hlen, proto, pad=int(rng.integers(0, 40)) if i % 4 == 1 else 0)
            arena[align + i * stride:align + i * stride + F] = np.frombuffer(fr, dtype=np.uint8)
            info.append((hlen, proto, i))
        off = align + np.arange(n, dtype=np.uint64) * stride
        ln = np.full(n, F, dtype=np.uint32)
        # torch allocations are 256-byte aligned: the frame start alignment mod 16 is `align`
        for flags in (tm.F_FCS, 0):
            key = ("band", F, stride, align, n)
            if align % 8 == 0:   # the variable and host forms (always the general kernel) on a sixth of the batches
                seen.add(check_all_forms(dev, oracle, inet_oracle, key, arena, off, ln, flags, info, fixed=(align, stride, F)))
                continue
            exp_a, exp_s, exp_f = reference(key, oracle, inet_oracle, arena, off, ln, flags)
            a, s, f, c, ptr = run_fixed(dev, arena, align, stride, F, n, flags, tm.L4_CSUM_SET)
            assert na.txs_last_launch() == na.txs_route(ptr, stride, F, n, flags)
            seen.add(na.txs_last_launch())
            assert_same(s, exp_s, (key, flags, "fixed status"), info)
            assert_same(f, exp_f, (key, flags, "fixed fields"), info)
            assert_same(a, exp_a, (key, flags, "fixed arena"), info, off, ln)
            assert c == int(np.count_nonzero(exp_s & np.uint32(tm.L4_CSUM_SET)))
    assert seen == ({"lds-dma"} if txs_kernel == "dma" else {"general"})


def test_lds_dma_band_covers_every_header_length_and_protocol(dev, oracle, inet_oracle, txs_kernel):
    """All eleven header lengths x three protocols at each of the 29 lengths, in one batch of 70
    frames per length (70 frames hold all 33 combinations; a stride that is not a multiple of 4 moves the
    starts)."""
    for F in range(1496, 1525):
        rng = np.random.default_rng(F)
        n, stride, align = 70, F + 4 + (F % 3), F % 16
        arena = rng.integers(0, 256, align + (n - 1) * stride + F + 4, dtype=np.uint8)
        info = []
        for i in range(n):
            hlen, proto = HLENS[i % 11], PROTOS[(i // 11 + F) % 3]
            arena[align + i * stride:align + i * stride + F] = np.frombuffer(raw_frame(rng, F, hlen, proto), dtype=np.uint8)
            info.append((hlen, proto))
        off = align + np.arange(n, dtype=np.uint64) * stride
        ln = np.full(n, F, dtype=np.uint32)
        exp_a, exp_s, exp_f = reference(("band33", F), oracle, inet_oracle, arena, off, ln, tm.F_FCS)
        a, s, f, c, _ = run_fixed(dev, arena, align, stride, F, n, tm.F_FCS, tm.L4_CSUM_SET)
        assert na.txs_last_launch() == ("lds-dma" if txs_kernel == "dma" else "general")
        assert_same(s, exp_s, ("band33 status", F), info)
        assert_same(f, exp_f, ("band33 fields", F), info)
        assert_same(a, exp_a, ("band33 arena", F), info, off, ln)
        assert c == n


# ---- 5. nothing else is written: without TXS_F_FCS the four bytes behind each frame stay ----
def test_without_the_fcs_flag_the_bytes_behind_a_frame_are_untouched(dev, oracle, inet_oracle, txs_golden):
    recs = txs_golden["frames"]
    arena = np.frombuffer(txs_golden["input_bytes"], dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    a, s, f, _ = run_dev(dev, arena, off, ln, 0)
    for o, l in zip(off, ln):
        e = int(o) + int(l)
        assert np.array_equal(a[e:e + 4], arena[e:e + 4])
    assert not np.any(s & tm.FCS_SET) and not np.any(f["fcs"])
    changed = np.nonzero(a != arena)[0]
    allowed = set()
    for r in recs:
        st = r["status"][0]
        if st & tm.IP_CSUM_SET:
            allowed |= {r["off"] + 24, r["off"] + 25}
            if st & tm.L4_CSUM_SET:
                q = r["off"] + 14 + (int(arena[r["off"] + 14]) & 15) * 4 + tm.L4_FIELD[(st >> 16) & 0xFF]
                allowed |= {q, q + 1}
    assert set(int(p) for p in changed) <= allowed


# ---- 6. consistency inside the library ----
@pytest.fixture(scope="module")
def mixed_batch():
    frames, info = straddle_batch()
    frames, info = frames[::5], info[::5]
    b2, i2 = border_batch()
    frames += b2[::7]
    info += i2[::7]
    return pack(frames, seed=11) + (info,)


def test_sealed_batches_pass_the_validator(dev, oracle, inet_oracle, mixed_batch):
    arena, off, ln, info = mixed_batch
    sealed, st, _, _ = run_dev(dev, arena, off, ln, tm.F_FCS)
    ln4 = (ln + 4).astype(np.uint32)
    key = "rxv-of-sealed"
    if key not in _REF:
        _REF[key] = rm.verdicts(oracle, inet_oracle, sealed, off, ln4, rm.F_TRAILER)
    exp = _REF[key]
    d = to_dev(sealed, dev)
    out = torch.full((len(off),), -1, dtype=torch.int32, device=dev)
    na.rx_validate_dev(d, sealed.nbytes, to_dev(off.view(np.int64), dev), to_dev(ln4.view(np.int32), dev), out, len(off),
                       flags=rm.F_TRAILER)
    torch.cuda.synchronize()
    got = out.cpu().numpy().view(np.uint32)
    assert_same(got, exp, "validator on sealed frames", info)
    assert not np.any(got & np.uint32(rm.FCS_BAD | rm.IP_BAD_CSUM | rm.L4_BAD_CSUM | rm.IP_BAD_HDR | rm.L4_SHORT))
    assert np.all(got & np.uint32(rm.L4_CHECKED))
    padded = np.array([p != 0 for (_, _, _, p) in info])
    assert np.array_equal((got & np.uint32(rm.IP_BAD_LEN)) != 0, padded)


def test_a_batch_without_ipv4_equals_the_tx_fcs_path(dev, mixed_batch):
    arena, off, ln, _ = mixed_batch
    plain = arena.copy()
    for o in off:
        plain[int(o) + 12] = 0x86   # no frame is IPv4 any more
    want = plain.copy()
    na.tx_batch_host(want, want.nbytes, off, ln, len(off))
    a, s, f, _ = run_dev(dev, plain, off, ln, tm.F_FCS)
    assert np.array_equal(a, want)
    assert np.all(s == tm.FCS_SET) and not np.any(f["ip_csum"]) and not np.any(f["l4_csum"])
    a, s, _ = run_host(plain, off, ln, tm.F_FCS)
    assert np.array_equal(a, want)
    # F = 0 and other edges: what ether_fcs_tx_batch_host writes for the same bytes
    edge = np.arange(64, dtype=np.uint8)
    eo = np.array([0, 8, 20, 40], dtype=np.uint64)
    el = np.array([0, 1, 13, 14], dtype=np.uint32)
    want = edge.copy()
    na.tx_batch_host(want, want.nbytes, eo, el, 4)
    a, s, _, _ = run_dev(dev, edge, eo, el, tm.F_FCS)
    assert np.array_equal(a, want)
    assert list(s) == [tm.FCS_SET | tm.RUNT] * 3 + [tm.FCS_SET]


def test_fields_equal_the_inet_and_fcs_paths_and_sealing_twice_changes_nothing(dev, oracle, inet_oracle, mixed_batch):
    arena, off, ln, info = mixed_batch
    n = len(off)
    sealed, st, fl, _ = run_dev(dev, arena, off, ln, tm.F_FCS)
    again, st2, fl2, _ = run_dev(dev, sealed, off, ln, tm.F_FCS)
    assert np.array_equal(again, sealed) and np.array_equal(st2, st) and np.array_equal(fl2, fl)
    # the FCS of the sealed bytes
    d = to_dev(sealed, dev)
    d_off = to_dev(off.view(np.int64), dev)
    out = torch.zeros(n, dtype=torch.int32, device=dev)
    na.batch_dev(d, sealed.nbytes, d_off, to_dev(ln.view(np.int32), dev), out, n)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), fl["fcs"])
    # the checksums of the sealed bytes with the fields zeroed
    z = sealed.copy()
    hl = np.array([h for (_, h, _, _) in info])
    pr = np.array([p for (_, _, p, _) in info])
    for o, (F, hlen, proto, pad) in zip(off, info):
        o = int(o)
        z[o + 24:o + 26] = 0
        q = o + 14 + hlen + tm.L4_FIELD[proto]
        z[q:q + 2] = 0
    dz = to_dev(z, dev)
    ipo = torch.zeros(n, dtype=torch.int16, device=dev)
    na.inet_batch_dev("ip", dz, z.nbytes, to_dev((off + 14).view(np.int64), dev), to_dev(hl.astype(np.uint32).view(np.int32), dev),
                      None, ipo, n)
    torch.cuda.synchronize()
    assert np.array_equal(ipo.cpu().numpy().view(np.uint16), fl["ip_csum"])
    for proto, mode in ((6, "tcp"), (17, "udp"), (1, "ip")):
        idx = np.nonzero(pr == proto)[0]
        assert len(idx) > 100
        soff = np.array([int(off[i]) + 14 + info[i][1] for i in idx], dtype=np.uint64)
        slen = np.array([info[i][0] - 14 - info[i][1] - info[i][3] for i in idx], dtype=np.uint32)
        addr = []
        for i in idx:
            s_raw, d_raw = np.frombuffer(z[int(off[i]) + 26:int(off[i]) + 34].tobytes(), dtype="<u4")
            addr += [socket.ntohl(int(s_raw)), socket.ntohl(int(d_raw))] if proto == 6 else [int(s_raw), int(d_raw)]
        o16 = torch.zeros(len(idx), dtype=torch.int16, device=dev)
        na.inet_batch_dev(mode, dz, z.nbytes, to_dev(soff.view(np.int64), dev), to_dev(slen.view(np.int32), dev),
                          None if mode == "ip" else to_dev(np.array(addr, dtype=np.uint32).view(np.int32), dev), o16, len(idx))
        torch.cuda.synchronize()
        got = o16.cpu().numpy().view(np.uint16)
        if proto == 17:
            got = np.where(got == 0, 0xFFFF, got).astype(np.uint16)   # RFC 768
        assert np.array_equal(got, fl["l4_csum"][idx]), mode


# ---- 7. count and count_mask, NULL status or fields, n = 0, a tiny arena, two threads ----
def test_counts_null_outputs_and_edges(dev, oracle, inet_oracle, txs_golden):
    recs = txs_golden["frames"]
    arena = np.frombuffer(txs_golden["input_bytes"], dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    exp_s = np.array([r["status"][1] for r in recs], dtype=np.uint32)
    exp_a = np.frombuffer(txs_golden["sealed_bytes"][1], dtype=np.uint8)
    for mask in (0, tm.FCS_SET, tm.RUNT | tm.IP_BAD_HDR | tm.IP_BAD_LEN | tm.FRAG | tm.L4_SHORT, tm.L4_CSUM_SET, 0xFFFFFFFF):
        a, s, f, c = run_dev(dev, arena, off, ln, tm.F_FCS, mask)
        assert c == int(np.count_nonzero(exp_s & np.uint32(mask))), hex(mask)
        assert run_host(arena, off, ln, tm.F_FCS, mask)[2] == c
    # NULL status, fields, count in every combination that drops one
    for kw in ({"status": False}, {"fields": False}, {"count": False}, {"status": False, "fields": False, "count": False}):
        a, s, f, c = run_dev(dev, arena, off, ln, tm.F_FCS, 0xFFFFFFFF, **kw)
        assert np.array_equal(a, exp_a), kw
        if s is not None:
            assert np.array_equal(s, exp_s)
    a = arena.copy()
    assert na.tx_seal_host(a, a.nbytes, off, ln, len(off), flags=tm.F_FCS, count_mask=tm.RUNT, status=None) == \
        int(np.count_nonzero(exp_s & tm.RUNT))
    assert np.array_equal(a, exp_a)
    # n = 0: nothing written, the count zeroed
    a, s, f, c = run_dev(dev, arena, off[:0], ln[:0], tm.F_FCS, 0xFFFFFFFF)
    assert c == 0 and np.array_equal(a, arena)
    d = to_dev(arena, dev)
    cnt = torch.full((1,), 9, dtype=torch.int64, device=dev)
    na.tx_seal_fixed_dev(d, 68, 64, 0, count=cnt)
    torch.cuda.synchronize()
    assert int(cnt.item()) == 0 and np.array_equal(d.cpu().numpy(), arena)
    assert na.tx_seal_host(arena, arena.nbytes, off, ln, 0) == 0
    # one-frame arenas shorter than two lane chunks (the guarded-load instantiation)
    small = [i for i, r in enumerate(recs) if r["len"] <= 150][:16]
    assert len(small) == 16
    for i in small:
        o, l = int(off[i]), int(ln[i])
        for flags in (tm.F_FCS, 0):
            one = arena[o:o + l + 4].copy()
            exp1 = np.frombuffer(txs_golden["sealed_bytes"][flags], dtype=np.uint8)[o:o + l + 4]
            a, s, f, _ = run_dev(dev, one, np.array([0], dtype=np.uint64), ln[i:i + 1], flags)
            assert np.array_equal(a, exp1), recs[i]["tag"]
            assert s[0] == recs[i]["status"][flags] and list(f[0]) == recs[i]["fields"][flags], recs[i]["tag"]
            a, s, f, c, _ = run_fixed(dev, one, 0, l + 4, l, 1, flags)
            assert np.array_equal(a, exp1) and s[0] == recs[i]["status"][flags], recs[i]["tag"]
    # a non-default stream
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        a, s, f, c = run_dev(dev, arena, off, ln, tm.F_FCS, tm.FCS_SET, stream=st)
    assert np.array_equal(a, exp_a) and c == len(off)


def test_two_threads_concurrently(dev, txs_golden):
    recs = txs_golden["frames"]
    arena = np.frombuffer(txs_golden["input_bytes"], dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    exp = [np.frombuffer(b, dtype=np.uint8) for b in txs_golden["sealed_bytes"]]
    errs = []

    def work(flags, use_host):
        try:
            torch.cuda.set_device(0)
            for _ in range(4):
                if use_host:
                    a = run_host(arena, off, ln, flags)[0]
                else:
                    s = torch.cuda.Stream()
                    with torch.cuda.stream(s):
                        a = run_dev(dev, arena, off, ln, flags, stream=s)[0]
                if not np.array_equal(a, exp[flags]):
                    errs.append((flags, use_host))
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=a) for a in ((1, False), (0, False), (3, True), (2, True))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
