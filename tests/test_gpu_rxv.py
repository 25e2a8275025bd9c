"""GPU tests of the one-pass RX validator (include/nstack_rxv.h) through the C ABI: every verdict
word bit-exact against the model (tests/rxv_model.py: the header's rules with the oracle's CRC and
checksums) and against the independently generated golden vectors."""
import importlib.util
import json
import os
import socket
import threading

import numpy as np
import pytest

import nstack_amd as na
import rxv_model as rm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
_spec = importlib.util.spec_from_file_location("make_rxv_golden", os.path.join(GOLDEN, "make_rxv_golden.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)   # the frame builders (independent RFC 1071 / zlib formulation)

MASKS = (0, rm.FCS_BAD, rm.IP_BAD_CSUM | rm.L4_BAD_CSUM, rm.RUNT | rm.IP_BAD_HDR | rm.IP_BAD_LEN | rm.FRAG | rm.L4_SHORT,
         0xFFFFFFFF)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def rxv_golden():
    with open(os.path.join(GOLDEN, "rxv_vectors.json")) as f:
        vec = json.load(f)
    with open(os.path.join(GOLDEN, vec["arena"]), "rb") as f:
        vec["arena_bytes"] = f.read()
    return vec


@pytest.fixture(params=["general", "dma"], autouse=True)
def rxv_kernel(request):
    """Every test runs under both DMA thresholds (identical verdicts required): general = 1 << 63, a
    quarter-wave per frame with register loads for every batch; dma = 0, fixed-stride batches whose
    geometry fits the LDS-DMA kernel's slots through rxv_dma_kernel. Variable and host batches always
    take the general kernel (rxv::route), so in this file only test_fixed_form's in-band shapes reach
    rxv_dma_kernel; tests/test_gpu_rxv_cuts.py holds the rest of that kernel's tests."""
    old = na.rx_validate_set_dma_threshold(0 if request.param == "dma" else (1 << 63))
    yield request.param
    na.rx_validate_set_dma_threshold(old)


def to_dev(arr, dev):
    return torch.from_numpy(np.ascontiguousarray(arr)).to(dev)


def run_dev(dev, arena, off, ln, flags, bad_mask=0, want_bad=True, stream=None):
    """(verdicts, bad count) of the variable device form."""
    n = len(off)
    d_arena = to_dev(arena, dev)
    d_off = to_dev(np.asarray(off, dtype=np.uint64).view(np.int64), dev)
    d_len = to_dev(np.asarray(ln, dtype=np.uint32).view(np.int32), dev)
    out = torch.full((max(n, 1),), -1, dtype=torch.int32, device=dev)
    bad = torch.full((1,), 77, dtype=torch.int64, device=dev) if want_bad else None
    na.rx_validate_dev(d_arena, arena.nbytes, d_off, d_len, out, n, flags=flags, bad_mask=bad_mask, bad=bad,
                       stream=stream)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32)[:n], (int(bad.item()) if want_bad else None)


def pack(frames, aligns=None, tail=16, seed=1):
    """Frames into one arena, frame i starting at aligns[i] mod 16 (random when None)."""
    rng = np.random.default_rng(seed)
    buf, off = bytearray(), []
    for i, fr in enumerate(frames):
        a = int(rng.integers(0, 16)) if aligns is None else aligns[i]
        buf.extend(bytes((a - len(buf)) % 16))
        off.append(len(buf))
        buf.extend(fr)
    buf.extend(rng.integers(0, 256, tail, dtype=np.uint8).tobytes())
    return (np.frombuffer(bytes(buf), dtype=np.uint8).copy(), np.array(off, dtype=np.uint64),
            np.array([len(f) for f in frames], dtype=np.uint32))


def names(v):
    return hex(int(v))


def assert_equal(got, exp, what, info=None):
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (what, len(bad), [(int(i), names(got[i]), names(exp[i]), info[i] if info else None)
                                            for i in bad[:8]])


# ---- 1. golden vectors and the pcap ----
@pytest.mark.parametrize("flags,key", [(rm.F_TRAILER, "expect_trailer"), (0, "expect_plain")])
def test_golden_dev_and_host(dev, rxv_golden, flags, key):
    recs = rxv_golden["frames"]
    arena = np.frombuffer(rxv_golden["arena_bytes"], dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    exp = np.array([r[key] for r in recs], dtype=np.uint32)
    tags = [r["tag"] for r in recs]
    for mask in MASKS:
        got, bad = run_dev(dev, arena, off, ln, flags, mask)
        assert_equal(got, exp, "dev", tags)
        assert bad == int(np.count_nonzero(exp & np.uint32(mask))), hex(mask)
        out = np.full(len(off), 0xDEADBEEF, dtype=np.uint32)
        hbad = na.rx_validate_host(arena, arena.nbytes, off, ln, out, len(off), flags=flags, bad_mask=mask)
        assert_equal(out, exp, "host", tags)
        assert hbad == bad


@pytest.mark.parametrize("flags,key", [(rm.F_TRAILER, "expect_trailer"), (0, "expect_plain")])
def test_golden_pcap(dev, rxv_golden, flags, key):
    arena, off, ln, lt = na.pcap_read(os.path.join(GOLDEN, rxv_golden["pcap"]))
    exp = np.array([r[key] for r in rxv_golden["pcap_frames"]], dtype=np.uint32)
    assert lt == 1 and len(off) == len(exp)
    got, bad = run_dev(dev, arena, off, ln, flags, rm.FCS_BAD | rm.L4_BAD_CSUM)
    assert_equal(got, exp, "pcap dev", [r["tag"] for r in rxv_golden["pcap_frames"]])
    assert bad == int(np.count_nonzero(exp & np.uint32(rm.FCS_BAD | rm.L4_BAD_CSUM)))
    out = np.zeros(len(off), dtype=np.uint32)
    assert na.rx_validate_host(arena, arena.nbytes, off, ln, out, len(off), flags=flags, bad_mask=rm.IPV4) == \
        int(np.count_nonzero(exp & np.uint32(rm.IPV4)))
    assert_equal(out, exp, "pcap host")


# ---- 2. built traffic, then one-byte corruptions ----
PAYLOADS = (0, 1, 2, 3, 17, 18, 19, 63, 64, 65, 1459, 1460)
PROTO = {"tcp": 6, "udp": 17, "icmp": 1}
L4HDR = {"tcp": 20, "udp": 8, "icmp": 8}


def built_traffic(trailer):
    """(frames, aligns, info): valid frames over start alignment x hlen x payload x protocol, and the
    padded cases. info[i] = (kind, hlen, l4 length, pad bytes)."""
    import random
    rng = random.Random(77 + trailer)
    frames, aligns, info = [], [], []
    for hlen in (20, 24, 40, 60):
        for n in PAYLOADS:
            for kind in ("tcp", "udp", "icmp"):
                for a in range(16):
                    frames.append(gen.l4_frame(kind, rng.randbytes(n), hlen, trailer=trailer, rng=rng))
                    aligns.append(a)
                    info.append((kind, hlen, L4HDR[kind] + n, 0))
    for kind in ("tcp", "udp", "icmp"):
        for n in (0, 1, 2, 3, 5):
            for a in range(16):
                fr = gen.l4_frame(kind, rng.randbytes(n), 20, pad_to=60, trailer=trailer, rng=rng)
                frames.append(fr)
                aligns.append(a)
                info.append((kind, 20, L4HDR[kind] + n, 60 - (14 + 20 + L4HDR[kind] + n)))
    return frames, aligns, info


@pytest.mark.parametrize("trailer", [True, False])
def test_built_traffic_is_clean_and_corruptions_flip_exactly_the_models_bits(dev, oracle, inet_oracle, trailer):
    flags = rm.F_TRAILER if trailer else 0
    frames, aligns, info = built_traffic(trailer)
    assert 2500 <= len(frames) <= 8000
    arena, off, ln = pack(frames, aligns)
    clean = np.array([rm.IPV4 | rm.L4_CHECKED | (PROTO[k] << 16) | (rm.IP_BAD_LEN if pad else 0)
                      for k, _, _, pad in info], dtype=np.uint32)
    assert_equal(rm.verdicts(oracle, inet_oracle, arena, off, ln, flags), clean, "model on clean traffic", info)
    got, bad = run_dev(dev, arena, off, ln, flags, 0xFFFF & ~(rm.IPV4 | rm.L4_CHECKED | rm.IP_BAD_LEN))
    assert_equal(got, clean, "clean traffic", list(zip(info, aligns)))
    assert bad == 0

    fcs = rm.FCS_BAD if trailer else 0
    regions = ["mac", "ip", "l4_first", "l4_mid", "l4_last"] + (["trailer"] if trailer else []) + ["pad"]
    for region in regions:
        sel, bent, exact = [], [], []
        for i, (fr, (kind, hlen, L, pad)) in enumerate(zip(frames, info)):
            l4 = 14 + hlen
            if region == "mac":
                pos, want = i % 12, clean[i] | fcs
            elif region == "ip":
                pos, want = 14 + (i % hlen), None          # vhl / len / foff / proto bytes: whatever the model says
            elif region == "l4_first":
                pos, want = l4, clean[i] | fcs | rm.L4_BAD_CSUM
            elif region == "l4_mid":
                pos, want = l4 + L // 2, clean[i] | fcs | rm.L4_BAD_CSUM
            elif region == "l4_last":
                pos, want = l4 + L - 1, clean[i] | fcs | rm.L4_BAD_CSUM
            elif region == "trailer":
                pos, want = len(fr) - 1 - (i % 4), clean[i] | fcs
            else:
                if not pad:
                    continue
                pos, want = l4 + L + (i % pad), clean[i] | fcs
            sel.append(i)
            bent.append(gen.flip(fr, pos))
            exact.append(want)
        a2, o2, l2 = pack(bent, [aligns[i] for i in sel])
        exp = rm.verdicts(oracle, inet_oracle, a2, o2, l2, flags)
        for q, want in enumerate(exact):
            if want is not None:
                assert exp[q] == want, (region, info[sel[q]], names(exp[q]), names(want))
        if region == "ip":   # every header byte breaks the header checksum or the header's shape
            assert all(e & (rm.IP_BAD_CSUM | rm.IP_BAD_HDR) for e in exp)
        got, _ = run_dev(dev, a2, o2, l2, flags)
        assert_equal(got, exp, region, [(info[i], aligns[i]) for i in sel])


# ---- 3. random bytes with forced header fields ----
def random_frames(seed, n=6000):
    rng = np.random.default_rng(seed)
    frames = []
    for i in range(n):
        r = rng.random()
        F = int(rng.integers(0, 80)) if r < 0.3 else int(rng.integers(0, 1700)) if r < 0.95 else int(rng.integers(1700, 9300))
        b = bytearray(rng.integers(0, 256, F, dtype=np.uint8).tobytes())
        T = 4
        if F >= 14 and rng.random() < 0.9:
            b[12:14] = b"\x08\x00"
        if F > 14:
            b[14] = int(rng.choice([0x45, 0x45, 0x46, 0x4A, 0x4F, 0x44, 0x35, 0x65]))
        if F > 23:
            b[23] = int(rng.choice([6, 6, 17, 17, 1, 47]))
        if F > 21 and rng.random() < 0.85:
            b[20:22] = bytes([int(rng.choice([0x00, 0x40])), 0])
        if F > 17:
            P = max(F - 14 - T, 0)
            hl = (b[14] & 15) * 4
            pick = rng.integers(0, 8)
            ipl = [P, P, P + 4, max(P - int(rng.integers(0, 50)), 0), hl, max(hl - 1, 0), hl + int(rng.integers(0, 24)),
                   int(rng.integers(0, 65536))][pick]
            b[16:18] = int(ipl & 0xFFFF).to_bytes(2, "big")
        q = 14 + (b[14] & 15) * 4 + 6 if F > 14 else F
        if q + 2 <= F and rng.random() < 0.2:
            b[q:q + 2] = b"\x00\x00"   # a UDP header's checksum field: "none sent"
        frames.append(bytes(b))
    return frames


@pytest.fixture(scope="module")
def random_batch(oracle, inet_oracle):
    frames = random_frames(4242)
    frames[-1] = frames[-1] + bytes(range(40))   # the last frame is not empty
    arena, off, ln = pack(frames, tail=0, seed=9)   # the last frame ends flush with the arena
    assert int(off[-1]) + int(ln[-1]) == arena.nbytes
    exp = {f: rm.verdicts(oracle, inet_oracle, arena, off, ln, f) for f in (rm.F_TRAILER, 0)}
    return arena, off, ln, exp


@pytest.mark.parametrize("flags", [rm.F_TRAILER, 0])
def test_random_bytes_with_forced_fields(dev, random_batch, flags):
    arena, off, ln, exp = random_batch
    e = exp[flags]
    for bit in (rm.RUNT, rm.IP_BAD_HDR, rm.IP_BAD_LEN, rm.IP_BAD_CSUM, rm.FRAG, rm.L4_CHECKED, rm.L4_SHORT):
        assert np.count_nonzero(e & np.uint32(bit)) > 10, hex(bit)   # the batch reaches every branch
    mask = rm.L4_BAD_CSUM | rm.L4_SHORT | rm.RUNT
    got, bad = run_dev(dev, arena, off, ln, flags, mask)
    assert_equal(got, e, "random", [(int(l), int(o) % 16) for o, l in zip(off, ln)])
    assert bad == int(np.count_nonzero(e & np.uint32(mask)))
    out = np.zeros(len(off), dtype=np.uint32)
    assert na.rx_validate_host(arena, arena.nbytes, off, ln, out, len(off), flags=flags, bad_mask=mask) == bad
    assert_equal(out, e, "random host")


# ---- 4. fixed form ----
@pytest.mark.parametrize("stride,length,trailer", [(1518, 1518, True), (1536, 1518, True), (2048, 1514, False),
                                                   (1519, 1517, True), (1524, 1524, True), (1496, 1496, True),
                                                   (64, 60, True), (9018, 9018, True)])
def test_fixed_form(dev, oracle, inet_oracle, rxv_kernel, stride, length, trailer):
    import random
    flags = rm.F_TRAILER if trailer else 0
    n = 501 if length > 4000 else 4001   # not a multiple of the four-frame item
    T = 4 if trailer else 0
    for base in (0, 1, 3):
        rng = random.Random(stride * 7 + length + base)
        buf = bytearray(rng.randbytes(base + n * stride))
        for i in range(n):
            kind = ("tcp", "udp", "icmp")[i % 3]
            pay = length - T - 14 - 20 - L4HDR[kind]
            fr = gen.l4_frame(kind, rng.randbytes(pay), 20, trailer=trailer, rng=rng)
            assert len(fr) == length
            if i % 4 == 3:
                fr = gen.flip(fr, rng.randrange(length))
            buf[base + i * stride:base + i * stride + length] = fr
        buf = buf[:base + (n - 1) * stride + length]   # the last frame ends the allocation
        arena = np.frombuffer(bytes(buf), dtype=np.uint8).copy()
        off = base + np.arange(n, dtype=np.uint64) * stride
        ln = np.full(n, length, dtype=np.uint32)
        exp = rm.verdicts(oracle, inet_oracle, arena, off, ln, flags)
        assert np.count_nonzero(exp == exp[0]) < n   # clean and bent frames
        d = to_dev(arena, dev)
        out = torch.full((n,), -1, dtype=torch.int32, device=dev)
        bad = torch.full((1,), 5, dtype=torch.int64, device=dev)
        mask = rm.FCS_BAD | rm.IP_BAD_CSUM | rm.L4_BAD_CSUM
        na.rx_validate_fixed_dev(d.data_ptr() + base, stride, length, n, out, flags=flags, bad_mask=mask, bad=bad)
        torch.cuda.synchronize()
        # in-band shapes actually went through the LDS-DMA kernel under the dma fixture
        in_band = 1496 <= length <= 1524 and stride <= 2048 and 3 * stride + length <= 6126
        assert na.rxv_route(d.data_ptr() + base, stride, length, n) == ("lds-dma" if rxv_kernel == "dma" and in_band else "general")
        assert na.rxv_last_launch() == ("lds-dma" if rxv_kernel == "dma" and in_band else "general")
        assert_equal(out.cpu().numpy().view(np.uint32), exp, (stride, length, base))
        assert int(bad.item()) == int(np.count_nonzero(exp & np.uint32(mask)))


# ---- 5. cross-check against the shipped paths on the same batch ----
def test_agrees_with_the_fcs_and_inet_paths(dev, oracle, inet_oracle, random_batch):
    arena, off, ln, _ = random_batch
    frames, aligns, _ = built_traffic(True)
    bent = [gen.flip(f, (7 * i) % len(f)) if i % 2 else f for i, f in enumerate(frames)]
    a2, o2, l2 = pack(bent, aligns)
    for A, O, L in ((arena, off, ln), (a2, o2, l2)):
        n = len(O)
        got, _ = run_dev(dev, A, O, L, rm.F_TRAILER)
        d_arena = to_dev(A, dev)
        d_off = to_dev(O.view(np.int64), dev)
        d_len = to_dev(L.view(np.int32), dev)
        ok = torch.zeros(n, dtype=torch.uint8, device=dev)
        bad = torch.zeros(1, dtype=torch.int64, device=dev)
        na.verify_dev(d_arena, A.nbytes, d_off, d_len, ok, bad, n)
        torch.cuda.synchronize()
        assert np.array_equal(got & rm.FCS_BAD, 1 - ok.cpu().numpy().astype(np.uint32))
        # the segments the model parsed, through inet_csum_batch_dev with the mode their protocol names
        buf = A.tobytes()
        parsed = []
        for i in range(n):
            p = []
            v = rm.verdict(oracle, inet_oracle, buf[int(O[i]):int(O[i]) + int(L[i])], rm.F_TRAILER, p)
            assert bool(p) == bool(v & rm.L4_CHECKED)
            parsed.append(p[0] if p else None)
        for proto, mode in ((6, "tcp"), (17, "udp"), (1, "ip")):
            idx, soff, slen, addr = [], [], [], []
            for i, q in enumerate(parsed):
                if q is not None and q.proto == proto:
                    idx.append(i)
                    soff.append(int(O[i]) + q.l4_off)
                    slen.append(q.l4_len)
                    addr += [socket.ntohl(q.src), socket.ntohl(q.dst)] if proto == 6 else [q.src, q.dst]
            assert len(idx) > 20, mode
            out = torch.zeros(len(idx), dtype=torch.int16, device=dev)
            na.inet_batch_dev(mode, d_arena, A.nbytes, to_dev(np.array(soff, dtype=np.uint64).view(np.int64), dev),
                              to_dev(np.array(slen, dtype=np.uint32).view(np.int32), dev),
                              None if mode == "ip" else to_dev(np.array(addr, dtype=np.uint32).view(np.int32), dev),
                              out, len(idx))
            torch.cuda.synchronize()
            nz = out.cpu().numpy().view(np.uint16) != 0
            assert np.array_equal((got[idx] & rm.L4_BAD_CSUM) != 0, nz), mode
            assert np.all(got[idx] & rm.L4_CHECKED)


# ---- 6. edge cases ----
def test_edge_cases(dev, rxv_golden):
    recs = rxv_golden["frames"]
    arena = np.frombuffer(rxv_golden["arena_bytes"], dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    exp = np.array([r["expect_trailer"] for r in recs], dtype=np.uint32)
    # n = 0: nothing written, the count zeroed
    got, bad = run_dev(dev, arena, off[:0], ln[:0], rm.F_TRAILER, 0xFFFFFFFF)
    assert bad == 0 and got.size == 0
    d = to_dev(arena, dev)
    badt = torch.full((1,), 9, dtype=torch.int64, device=dev)
    na.rx_validate_fixed_dev(d, 64, 64, 0, None, bad=badt)
    torch.cuda.synchronize()
    assert int(badt.item()) == 0
    assert na.rx_validate_host(arena, arena.nbytes, off, ln, None, 0) == 0
    # bad = NULL; bad_mask = 0
    got, _ = run_dev(dev, arena, off, ln, rm.F_TRAILER, 0xFFFFFFFF, want_bad=False)
    assert_equal(got, exp, "bad = NULL")
    got, bad = run_dev(dev, arena, off, ln, rm.F_TRAILER, 0)
    assert bad == 0
    # a single frame, and a one-frame arena shorter than two lane chunks (guarded loads)
    for i in (0, len(recs) // 2):
        o, l = int(off[i]), int(ln[i])
        got, _ = run_dev(dev, arena[o:o + l].copy(), np.array([0], dtype=np.uint64), ln[i:i + 1], rm.F_TRAILER)
        assert got[0] == exp[i], recs[i]["tag"]
    small = [i for i, r in enumerate(recs) if r["len"] <= 100][:12]
    for i in small:
        o, l = int(off[i]), int(ln[i])
        got, _ = run_dev(dev, arena[o:o + max(l, 1)].copy(), np.array([0], dtype=np.uint64), ln[i:i + 1], rm.F_TRAILER)
        assert got[0] == exp[i], recs[i]["tag"]
    # a non-default stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        got, bad = run_dev(dev, arena, off, ln, rm.F_TRAILER, rm.FCS_BAD, stream=s)
    assert_equal(got, exp, "stream")
    assert bad == int(np.count_nonzero(exp & rm.FCS_BAD))


def test_two_threads_concurrently(dev, rxv_golden):
    recs = rxv_golden["frames"]
    arena = np.frombuffer(rxv_golden["arena_bytes"], dtype=np.uint8).copy()
    off = np.array([r["off"] for r in recs], dtype=np.uint64)
    ln = np.array([r["len"] for r in recs], dtype=np.uint32)
    exp = {rm.F_TRAILER: np.array([r["expect_trailer"] for r in recs], dtype=np.uint32),
           0: np.array([r["expect_plain"] for r in recs], dtype=np.uint32)}
    errs = []

    def work(flags, use_host):
        try:
            torch.cuda.set_device(0)
            for _ in range(4):
                if use_host:
                    out = np.zeros(len(off), dtype=np.uint32)
                    na.rx_validate_host(arena, arena.nbytes, off, ln, out, len(off), flags=flags)
                else:
                    s = torch.cuda.Stream()
                    with torch.cuda.stream(s):
                        out, _ = run_dev(dev, arena, off, ln, flags, 0, stream=s)
                if not np.array_equal(out, exp[flags]):
                    errs.append((flags, use_host))
        except Exception as e:   # noqa: BLE001
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=a) for a in ((rm.F_TRAILER, False), (0, False), (rm.F_TRAILER, True), (0, True))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
