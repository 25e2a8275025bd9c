"""GPU tests of the RX validator's tail subtraction and of rxv_dma_kernel's verdicts.

Both kernels take the L4 sum as total - [0, 14 + hlen) - [14 + ip_len, F). The last term (per-word
masks, gated 6-word blocks, per-lane and per-segment geometry) shows only in a frame whose L4
checksum is valid and whose tail is not zero, so these tests move the cut cl = 14 + ip_len through
frames that hold a good datagram in front of non-zero bytes (tests/rxv_traffic.py), each cut with
a bent byte on either side of it, and compare every verdict word bit-exactly with the verdict the
frame was built for (tests/test_rxv_traffic.py checks those against the model and the independent
witness on the CPU). The LDS-DMA kernel, which only fixed-stride batches reach, also gets every
verdict class at every length of its band, every start alignment mod 16, batches whose slots are all
clamped to the arena's end and last items of 1 to 4 frames. Every launch meant for a kernel asserts
the kernel that ran."""
import contextlib

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm
import rxv_traffic as rt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GENERAL, DMA = 1 << 63, 0          # DMA thresholds that choose the kernel of a fixed-stride batch
DEFECTS = 0xFFFF & ~(rm.IPV4 | rm.L4_CHECKED)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


@contextlib.contextmanager
def dma_threshold(frames):
    old = na.rx_validate_set_dma_threshold(frames)
    try:
        yield
    finally:
        na.rx_validate_set_dma_threshold(old)


def flags_of(trailer):
    return rm.F_TRAILER if trailer else 0


def lay_out(M, stride, seed=5):
    """The rows of M (n frames of F bytes) at the given stride, random bytes between them; ends with the last frame."""
    n, F = M.shape
    if stride == F:
        return M.reshape(-1)
    buf = np.random.default_rng(seed).integers(1, 256, (n, stride), dtype=np.uint8)
    buf[:, :F] = M
    return buf.reshape(-1)[:(n - 1) * stride + F]


def place(dev, host, base, tail=0):
    """The bytes on the device behind `base` random bytes (and in front of `tail`): the allocation
    ends with the last frame when tail = 0."""
    rng = np.random.default_rng(base + 1)
    parts = [rng.integers(1, 256, base, dtype=np.uint8), host, rng.integers(1, 256, tail, dtype=np.uint8)]
    return torch.from_numpy(np.concatenate(parts)).to(dev)


def run_fixed(dev, d, base, stride, F, n, flags, mask, threshold, want):
    """Verdicts and bad count of the fixed form on the frames at d[base + i * stride]; asserts the
    route taken (`want`), both as predicted and as launched."""
    out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    bad = torch.full((1,), 5, dtype=torch.int64, device=dev)
    with dma_threshold(threshold):
        assert na.rxv_route(d.data_ptr() + base, stride, F, n) == want, (base, stride, F, n)
        na.rx_validate_fixed_dev(d.data_ptr() + base, stride, F, n, out, flags=flags, bad_mask=mask, bad=bad)
        torch.cuda.synchronize()
        assert na.rxv_last_launch() == want, (base, stride, F, n)
    return out.cpu().numpy().view(np.uint32), int(bad.item())


def run_var(dev, d, off, ln, flags, mask):
    """Verdicts and bad count of the variable device form (always the general kernel)."""
    n = len(off)
    d_off = torch.from_numpy(np.ascontiguousarray(off, dtype=np.uint64).view(np.int64)).to(dev)
    d_len = torch.from_numpy(np.ascontiguousarray(ln, dtype=np.uint32).view(np.int32)).to(dev)
    out = torch.full((n,), -1, dtype=torch.int32, device=dev)
    bad = torch.full((1,), 5, dtype=torch.int64, device=dev)
    na.rx_validate_dev(d, d.numel(), d_off, d_len, out, n, flags=flags, bad_mask=mask, bad=bad)
    torch.cuda.synchronize()
    assert na.rxv_last_launch() == "general"
    return out.cpu().numpy().view(np.uint32), int(bad.item())


def assert_equal(got, exp, what, info=None):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, len(bad), [(int(i), hex(int(got[i])), hex(int(exp[i])), info[i] if info else None)
                                            for i in bad[:8]])


def count(exp, mask):
    return int(np.count_nonzero(exp & np.uint32(mask)))


# ---- C1. every cut through the LDS-DMA kernel ----
@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", rt.DMA_LENGTHS)
def test_every_cut_through_the_lds_dma_kernel(dev, F, trailer):
    sw = rt.full_sweep(F, trailer)
    n, M = len(sw), sw.matrix()
    assert n > 25000
    nlast = sw.count("last")
    assert count(sw.expect, rm.L4_BAD_CSUM) == nlast == n - sw.count("clean") - sw.count("behind")
    wide = (6126 - F) // 3   # the widest stride whose four frames fit a slot
    for stride, bases in ((F, (0, 1, 2, 3, 13)), (wide, (5,))):
        host = lay_out(M, stride)
        for base in bases:
            got, bad = run_fixed(dev, place(dev, host, base), base, stride, F, n, flags_of(trailer), rm.L4_BAD_CSUM,
                                 DMA, "lds-dma")
            assert_equal(got, sw.expect, (F, stride, base), sw.info)
            assert bad == nlast


# ---- C2. the same sweeps through the general kernel, fixed and variable form ----
def general_both_forms(dev, sw, F, trailer):
    n, host = len(sw), sw.matrix().reshape(-1)
    nlast = sw.count("last")
    for base in (0, 1, 2, 3):
        d = place(dev, host, base)
        got, bad = run_fixed(dev, d, base, F, F, n, flags_of(trailer), rm.L4_BAD_CSUM, GENERAL, "general")
        assert_equal(got, sw.expect, ("fixed", F, base), sw.info)
        assert bad == nlast
        got, bad = run_var(dev, d, base + np.arange(n, dtype=np.uint64) * F, np.full(n, F, dtype=np.uint32),
                           flags_of(trailer), rm.L4_BAD_CSUM)
        assert_equal(got, sw.expect, ("variable", F, base), sw.info)
        assert bad == nlast


@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", rt.FULL_LENGTHS)
def test_every_cut_through_the_general_kernel(dev, F, trailer):
    sw = rt.full_sweep(F, trailer)
    assert len(sw) > (25000 if F > 1000 else 10)
    general_both_forms(dev, sw, F, trailer)


@pytest.mark.parametrize("kind", rt.KINDS)
@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", rt.SEG_LENGTHS)
def test_cuts_at_segment_and_chunk_borders(dev, F, trailer, kind):
    sw = rt.seg_sweep(F, trailer, kind)
    assert len({cl for _, _, cl, _ in sw.info}) >= 500
    general_both_forms(dev, sw, F, trailer)


# ---- C3. variable mix ----
def pack(frames, seed):
    """Frames into one arena at random start alignments mod 16; the last frame ends the arena."""
    rng = np.random.default_rng(seed)
    buf, off = bytearray(), []
    for fr in frames:
        buf.extend(rng.integers(1, 256, (int(rng.integers(0, 16)) - len(buf)) % 16, dtype=np.uint8).tobytes())
        off.append(len(buf))
        buf.extend(fr)
    return (np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64),
            np.array([len(f) for f in frames], dtype=np.uint32))


@pytest.mark.parametrize("trailer", [True, False])
def test_variable_mix_dev_and_host(dev, oracle, inet_oracle, trailer):
    sw = rt.variable_mix(6000, trailer, seed=31 + trailer)
    arena, off, ln = pack(sw.frames, seed=3)
    assert int(off[-1]) + int(ln[-1]) == arena.nbytes and len(set(int(o) % 16 for o in off)) == 16
    d = torch.from_numpy(arena).to(dev)
    for flags in (flags_of(trailer), flags_of(not trailer)):
        exp = rm.verdicts(oracle, inet_oracle, arena, off, ln, flags)
        if flags == flags_of(trailer):
            assert_equal(exp, sw.expect, "model against the constructed verdicts", sw.info)
            assert count(exp, DEFECTS & ~rm.IP_BAD_LEN) == 0
        mask = rm.L4_BAD_CSUM | rm.IP_BAD_LEN
        got, bad = run_var(dev, d, off, ln, flags, mask)
        assert_equal(got, exp, ("dev", flags), list(zip(sw.info, ln, off % 16)))
        assert bad == count(exp, mask)
        out = np.full(len(off), 0xDEADBEEF, dtype=np.uint32)
        assert na.rx_validate_host(arena, arena.nbytes, off, ln, out, len(off), flags=flags, bad_mask=mask) == bad
        assert_equal(out, exp, ("host", flags), list(zip(sw.info, ln, off % 16)))


# ---- C4. quirks: tails that sum to 0 and to a multiple of 0xffff, the all-zero ICMP message ----
@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", [1518, 1600])
def test_quirk_frames(dev, F, trailer):
    sw = rt.quirk_frames(F, trailer)
    n, host = len(sw), sw.matrix().reshape(-1)
    assert n == 32 and count(sw.expect, rm.L4_BAD_CSUM | rm.FCS_BAD) == 0
    for base in (0, 1, 6, 15):
        d = place(dev, host, base)
        routes = [(GENERAL, "general")] + ([(DMA, "lds-dma")] if F == 1518 else [])
        for threshold, want in routes:
            got, bad = run_fixed(dev, d, base, F, F, n, flags_of(trailer), DEFECTS & ~rm.IP_BAD_LEN, threshold, want)
            assert_equal(got, sw.expect, (want, F, base), sw.info)
            assert bad == 0
        got, _ = run_var(dev, d, base + np.arange(n, dtype=np.uint64) * F, np.full(n, F, dtype=np.uint32),
                         flags_of(trailer), 0)
        assert_equal(got, sw.expect, ("variable", F, base), sw.info)


# ---- C5. the LDS-DMA kernel's geometry with every verdict class ----
def dma_strides(F):
    return sorted({F, F + 1, F + 2, F + 3, (6126 - F) // 3})


DMA_BATCHES = (9, 10, 11, 12, 70, 259)   # last items of 1, 2, 3, 4, 2 and 3 frames; 9..12: every slot clamped


@pytest.mark.parametrize("F,trailer", [(F, True) for F in range(1496, 1525)] + [(F, False) for F in (1496, 1517, 1524)])
def test_dma_geometry_with_every_verdict_class(dev, oracle, inet_oracle, F, trailer):
    flags = flags_of(trailer)
    seen = 0
    for n in DMA_BATCHES:
        frames = rt.mixed_fixed(F, n, trailer, seed=1000 * F + n)
        M = np.frombuffer(b"".join(frames), dtype=np.uint8).reshape(n, F)
        for stride in dma_strides(F):
            host = lay_out(M, stride, seed=stride)
            off = np.arange(n, dtype=np.uint64) * stride
            exp = rm.verdicts(oracle, inet_oracle, host, off, np.full(n, F, dtype=np.uint32), flags)
            seen |= int(np.bitwise_or.reduce(exp))
            for base in range(16):
                d = place(dev, host, base)
                assert d.numel() == base + (n - 1) * stride + F   # the buffer ends with the last frame
                got, bad = run_fixed(dev, d, base, stride, F, n, flags, DEFECTS, DMA, "lds-dma")
                assert_equal(got, exp, (F, stride, n, base))
                assert bad == count(exp, DEFECTS)
    every = rm.IP_BAD_HDR | rm.IP_BAD_LEN | rm.IP_BAD_CSUM | rm.FRAG | rm.L4_BAD_CSUM | rm.L4_SHORT | (rm.FCS_BAD if trailer else 0)
    assert (seen & DEFECTS) == every, hex(seen)   # each defect a frame of this length can have (not RUNT)


# ---- C6. the general kernel's fixed form at small and edge shapes ----
@pytest.mark.parametrize("trailer", [True, False])
@pytest.mark.parametrize("F", [0, 3, 17, 18, 37, 38, 59, 60, 96, 97, 1535, 1536, 1537, 3072, 3073])
def test_general_fixed_form_small_and_edge_shapes(dev, oracle, inet_oracle, F, trailer):
    flags = flags_of(trailer)
    for n in (1, 2, 3, 33):
        frames = rt.mixed_fixed(F, n, trailer, seed=F + n) if F >= 38 else rt.tiny_fixed(F, n, seed=F + n)
        M = np.frombuffer(b"".join(frames), dtype=np.uint8).reshape(n, F)
        for stride in (F or 4, F + 5):
            host = lay_out(M, stride)
            exp = rm.verdicts(oracle, inet_oracle, host, np.arange(n, dtype=np.uint64) * stride,
                              np.full(n, F, dtype=np.uint32), flags)
            if F < 14 + (4 if trailer else 0):
                assert np.all(exp & rm.RUNT)
            for base in range(4):
                d = place(dev, host, base, tail=0 if F else 4)   # an empty allocation has no address
                got, bad = run_fixed(dev, d, base, stride, F, n, flags, DEFECTS, GENERAL, "general")
                assert_equal(got, exp, (F, stride, n, base))
                assert bad == count(exp, DEFECTS)


# ---- C7. the three routes agree ----
@pytest.mark.parametrize("trailer", [True, False])
def test_three_routes_give_identical_words(dev, oracle, inet_oracle, trailer):
    flags, n = flags_of(trailer), 70
    for F in range(1496, 1525):
        stride, base = F + 1, F % 16
        frames = rt.mixed_fixed(F, n, trailer, seed=1000 * F + n)
        host = lay_out(np.frombuffer(b"".join(frames), dtype=np.uint8).reshape(n, F), stride)
        d = place(dev, host, base)
        dma, bad_dma = run_fixed(dev, d, base, stride, F, n, flags, DEFECTS, DMA, "lds-dma")
        gen, bad_gen = run_fixed(dev, d, base, stride, F, n, flags, DEFECTS, GENERAL, "general")
        off = base + np.arange(n, dtype=np.uint64) * stride
        var, bad_var = run_var(dev, d, off, np.full(n, F, dtype=np.uint32), flags, DEFECTS)
        assert_equal(dma, gen, ("lds-dma against general", F))
        assert_equal(var, gen, ("variable against fixed", F))
        assert bad_dma == bad_gen == bad_var
        assert_equal(gen, rm.verdicts(oracle, inet_oracle, d.cpu().numpy(), off, np.full(n, F, dtype=np.uint32), flags),
                     ("model", F))
