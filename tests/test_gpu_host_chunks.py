"""GPU tests of the host forms inet_csum_batch_host, ether_rx_validate_host and ether_tx_seal_host
across the chunks of their double-buffered pipelines: batches sized by the engines' own bounds so
that a call takes a second and a third chunk (both slots, slot 0 reused), every cutting bound
(packets, bytes, the span rule), and both staging kinds (one dense span copy, gathered frames).
Every case asserts the chunk composition with tests/host_chunks.py first, runs the host form once
and compares all it returns or writes (for the sealer the whole arena, canary gaps included) with
the reference: the C oracle for inet, and for the validator and the sealer the model's results on one
block of frames, tiled (the model's results do not depend on where a frame lies). Then the error
return in mid-pipeline and the host forms' argument errors.

Host chunks are variable batches: the validator and the sealer always take the general kernel."""
import functools

import numpy as np
import pytest

import host_chunks as hc
import nstack_amd as na
import rxv_model as rm
import rxv_traffic as rt
import txs_model as tm
from test_gpu_txs import L4MIN, PROTOS, raw_frame

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

P = 1 << 20
LAYOUTS = ("A", "A'", "B", "C", "D", "E", "Z")
RXV_MASKS = (rm.FCS_BAD, rm.L4_BAD_CSUM | rm.RUNT)
TXS_MASK = tm.L4_CSUM_SET | tm.RUNT


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    torch.cuda.set_device(0)
    na.load()
    return torch.device("cuda:0")


def bounds(engine):
    k = hc.engine_constants(engine)
    assert k["kChunkPkts"] == P and k["kDepth"] == 2
    return k["kChunkBytes"]


# ---- the layouts: one block of frames (lengths, places, size), tiled ----
class Geometry:
    """Block frame j: ln[j] bytes at rel[j] from the block's start; the arena is `lead` bytes and then
    blocks of `size` bytes; the batch is the first n frames of the tiled blocks, in `order`."""

    def __init__(self, ln, slot, lead, n, order="asc", odd=True):
        self.ln, self.lead, self.n, self.order = np.asarray(ln, dtype=np.int64), lead, n, order
        slot = np.asarray(slot, dtype=np.int64)
        self.rel = np.cumsum(slot) - slot
        self.size = int(slot.sum())
        if odd and self.size % 2 == 0:   # alignment walks through every residue mod 16 from block to block
            self.size += 1
        self.m = len(self.ln)


def geometry(layout, K, T, top):
    """The layouts A..E (Z is made by zero_batch). `top`: the largest small frame of A."""
    rng = np.random.default_rng(sum(map(ord, layout)) * 4096 + T)
    if layout in ("A", "A'", "A2"):    # small frames packed, T bytes free behind each: the packet bound
        ln = rng.integers(0, top + 1, 4099)
        n = {"A": 2 * P + 77, "A'": 3 * P + 77, "A2": P + 77}[layout]
        return Geometry(ln, ln + T, 3, n, "perm" if layout == "A'" else "asc")
    if layout == "B":                  # exact fill: K / 1024 frames are K bytes of sum and of span, at lo & 15 == 15
        assert K % 1024 == 0 and (K // 1024) % 52
        return Geometry(np.full(52, 1024 - T), np.full(52, 1024), 15, 2 * (K // 1024) + 5, odd=False)
    j = np.arange(263)                 # two lengths, each often enough for every class of rxv_traffic.mixed_fixed
    ln = (1518 - j % 2) if layout == "E" else (1063 + 74 * (j % 2))
    ln[[7, 71, 200]] = 9000            # several 1536-byte segments
    ln[[3, 40, 99, 150]] = (10, 60, 77, 0)
    if layout == "C":                  # span less than twice the bytes: the span rule cuts, chunks stay dense
        slot = ((ln + T) / 0.55).astype(np.int64)
        return Geometry(ln, slot, 7, int(2.05 * K / slot.mean()))
    if layout == "D":                  # span more than twice the bytes: no cut, the chunk is gathered
        slot = np.ceil((ln + T) / 0.46).astype(np.int64)
        return Geometry(ln, slot, 9, int(1.02 * K / (ln + T).mean()))
    assert layout == "E"               # descending offsets, four bytes behind each frame
    return Geometry(ln, ln + 4, 11, int(1.2 * K / (ln + 4).mean()), "desc")


class Batch:
    """arena, off[], len[] of a layout; frame i is block frame which[i]. block/block_off/block_ln: one
    block as a batch of its own (what the per-frame models are evaluated on)."""

    def tiled(self, block_after):
        """The arena after a call that left every used frame's block bytes as in `block_after`."""
        exp = self.arena.copy()
        body = exp[self.lead:]
        body[:] = np.tile(block_after, self.reps)
        if self.unused_from is not None:   # the last block's frames behind the batch's last one
            body[self.unused_from:] = self.arena[self.lead + self.unused_from:]
        return exp


def tiled_batch(layout, K, T, top, frames_of=None, tail_ok=None):
    g = geometry(layout, K, T, top)
    rng = np.random.default_rng(g.n)
    block = rng.integers(0, 256, g.size, dtype=np.uint8)   # canary bytes wherever no frame lies
    if frames_of is not None:
        frames = frames_of([int(x) for x in g.ln])
        if tail_ok is not None:   # equal slots (layout B): turn the block until the short last chunk holds what the case needs
            tail = [int(w) for w in np.arange(g.n - g.n % (K // 1024), g.n) % g.m]
            r = next(r for r in range(g.m) if tail_ok([frames[(w - r) % g.m] for w in tail]))
            frames = [frames[(w - r) % g.m] for w in range(g.m)]
        for r, f in zip(g.rel, frames):
            block[int(r):int(r) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    b = Batch()
    b.layout, b.lead, b.reps = layout, g.lead, -(-g.n // g.m)
    b.arena = np.concatenate([rng.integers(0, 256, g.lead, dtype=np.uint8), np.tile(block, b.reps)])
    i = np.arange(g.n)
    if g.order == "perm":
        i = rng.permutation(g.n)
    elif g.order == "desc":
        i = i[::-1]
    b.which = i % g.m
    b.off = (g.lead + (i // g.m) * g.size + g.rel[b.which]).astype(np.uint64)
    b.ln = g.ln[b.which].astype(np.uint32)
    b.n = g.n
    b.block, b.block_off, b.block_ln = block, g.rel.astype(np.uint64), g.ln.astype(np.uint32)
    b.unused_from = None if g.n % g.m == 0 else (b.reps - 1) * g.size + int(g.rel[g.n % g.m])
    return b


def zero_batch(T, frames_of=None):
    """Layout Z: P frames of length 0 at offset 0 (a whole chunk without a byte to copy), then 77
    frames of 60 bytes from offset 8, 67 apart."""
    rng = np.random.default_rng(26)
    b = Batch()
    b.layout, b.lead, b.reps, b.unused_from = "Z", 0, 1, None
    b.block_off = np.concatenate([[0], 8 + 67 * np.arange(77)]).astype(np.uint64)
    b.block_ln = np.array([0] + [60] * 77, dtype=np.uint32)
    b.block = rng.integers(0, 256, 8 + 67 * 77 + 5, dtype=np.uint8)
    if frames_of is not None:
        for r, f in zip(b.block_off, frames_of([int(x) for x in b.block_ln])):
            b.block[int(r):int(r) + len(f)] = np.frombuffer(f, dtype=np.uint8)
    b.arena = b.block.copy()
    b.which = np.concatenate([np.zeros(P, dtype=np.int64), 1 + np.arange(77)])
    b.off, b.ln, b.n = b.block_off[b.which], b.block_ln[b.which], P + 77
    return b


def chunks_of(b, K, T):
    b.chunks = hc.host_chunks(b.off, b.ln, K, P, T)
    return [(e - i, bound, staging) for i, e, bound, staging, _, _ in b.chunks]


def assert_composition(b, K, T):
    """The chunks the engine will form are the ones the layout is there for."""
    c = chunks_of(b, K, T)
    how = [x[1:] for x in c]
    if b.layout == "A":
        assert c == [(P, "pkts", "dense"), (P, "pkts", "dense"), (77, "end", "dense")]
    elif b.layout == "A'":
        assert c == [(P, "pkts", "gather")] * 3 + [(77, "end", "gather")]
    elif b.layout == "A2":
        assert c == [(P, "pkts", "dense"), (77, "end", "dense")]
    elif b.layout == "B":
        assert c == [(K // 1024, "bytes", "dense")] * 2 + [(5, "end", "dense")]
        for i, e, _, _, total, span in b.chunks[:2]:
            assert total == span == K
        assert all(int(b.off[i]) & 15 == 15 for i, *_ in b.chunks)   # K + 15 bytes in the staging buffer
    elif b.layout == "C":
        assert how == [("span", "dense"), ("span", "dense"), ("end", "dense")]
    elif b.layout == "D":
        assert how == [("bytes", "gather"), ("end", "dense")]
    elif b.layout == "E":
        assert len(c) == 2 and all(s == "dense" for _, _, s in c) and c[0][1] in ("bytes", "span")
        assert np.all(np.diff(b.off.astype(np.int64)) < 0)
    else:
        assert b.layout == "Z" and c == [(P, "pkts", "dense"), (77, "end", "dense")]
        assert b.chunks[0][4:] == (T * P, T)   # T = 0: not one byte to copy


def chunk_of(b, i):
    return next(k for k, c in enumerate(b.chunks) if c[0] <= i < c[1])


def assert_words(b, got, exp, what, fmt=hex):
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, (what, b.layout, int(bad.size), "frame, chunk, off, len, got, expected",
                           [(int(i), chunk_of(b, int(i)), int(b.off[i]), int(b.ln[i]), fmt(int(got[i])), fmt(int(exp[i])))
                            for i in bad[:6]], "chunks", [c[:4] for c in b.chunks])


def assert_arena(b, got, exp, what):
    bad = np.flatnonzero(got != exp)
    if bad.size:
        order = np.argsort(b.off, kind="stable")
        who = [int(order[max(int(np.searchsorted(b.off[order], p, side="right")) - 1, 0)]) for p in bad[:6]]
        raise AssertionError((what, b.layout, "bytes differ", int(bad.size), "byte, frame, chunk, at, len, got, expected",
                              [(int(p), i, chunk_of(b, i), int(p) - int(b.off[i]), int(b.ln[i]), int(got[p]), int(exp[p]))
                               for p, i in zip(bad[:6], who)]))


def selected_in_every_chunk(b, exp, mask):
    per = [int(np.count_nonzero(exp[i:e] & np.uint32(mask))) for i, e, *_ in b.chunks]
    assert all(per), (b.layout, hex(mask), per)   # so the sum over chunks is no single chunk's count
    return sum(per)


# ---- inet ----
def inet_batch(layout):
    return zero_batch(0) if layout == "Z" else tiled_batch(layout, bounds("inet"), 0, 120)


@functools.lru_cache(maxsize=1)
def inet_case(layout):
    b = inet_batch(layout)
    b.addr = np.random.default_rng(5).integers(0, 1 << 32, (b.n, 2), dtype=np.uint32)
    return b


def oracle_batch(o, mode, arena, off, ln, addr):
    out = np.empty(len(off), dtype=np.uint16)
    o.oracle_inet_batch(na.INET_MODES[mode], arena.ctypes.data, off.ctypes.data, ln.ctypes.data,
                        None if addr is None else addr.ctypes.data, out.ctypes.data, len(off))
    return out


def run_inet(b, mode):
    out = np.full(b.n, 0xA5A5, dtype=np.uint16)
    na.inet_batch_host(mode, b.arena, b.arena.nbytes, b.off, b.ln, None if mode == "ip" else b.addr, out, b.n)
    return out


INET_CASES = sorted([(layout, "tcp") for layout in LAYOUTS] + [(layout, m) for layout in ("A'", "B") for m in ("ip", "udp")])


@pytest.mark.parametrize("layout,mode", INET_CASES)
def test_inet_host_chunks(dev, inet_oracle, layout, mode):
    b = inet_case(layout)
    assert_composition(b, bounds("inet"), 0)
    exp = oracle_batch(inet_oracle, mode, b.arena, b.off, b.ln, None if mode == "ip" else b.addr)
    assert_words(b, run_inet(b, mode), exp, ("inet", mode))


# ---- the validator ----
def rxv_frames(lens):
    """A frame of each length in `lens`: per length, traffic that cycles through every verdict class."""
    out = [None] * len(lens)
    for F in sorted(set(lens)):
        idx = [j for j, x in enumerate(lens) if x == F]
        fr = rt.mixed_fixed(F, len(idx), True, seed=F) if F >= 38 else rt.tiny_fixed(F, len(idx), seed=F)
        for j, f in zip(idx, fr):
            out[j] = f
    return out


@functools.lru_cache(maxsize=1)
def rxv_case(layout, oracle, inet_oracle):
    def tail_ok(frames):
        v = np.array([rm.verdict(oracle, inet_oracle, f) for f in frames], dtype=np.uint32)
        return all(np.any(v & np.uint32(m)) for m in RXV_MASKS)

    K = bounds("rxv")
    b = zero_batch(0, rxv_frames) if layout == "Z" else tiled_batch(layout, K, 0, 60, rxv_frames,
                                                                    tail_ok if layout == "B" else None)
    b.block_exp = rm.verdicts(oracle, inet_oracle, b.block, b.block_off, b.block_ln, rm.F_TRAILER)
    return b


def assert_rxv_classes(b):
    """The block holds every verdict class its lengths admit."""
    v, F = b.block_exp, b.block_ln
    hlen = np.array([(int(b.block[int(o) + 14]) & 15) * 4 if l > 14 else 0 for o, l in zip(b.block_off, F)])
    checked = (v & rm.L4_CHECKED) != 0
    assert np.any((v & rm.FCS_BAD) != 0) and np.any((v & rm.FCS_BAD) == 0)
    assert np.any(((v & (rm.IPV4 | rm.RUNT)) == 0) & (F >= 18))                 # not IPv4
    assert np.any((v & rm.IP_BAD_HDR) != 0) and np.any((v & rm.FRAG) != 0)
    if F.min() < 18:
        assert np.any((v & rm.RUNT) != 0)
    for proto in (6, 17, 1):
        mine = checked & ((v >> rm.PROTO_SHIFT) & 0xFF == proto)
        assert np.any(mine & ((v & rm.L4_BAD_CSUM) == 0)) and np.any(mine & ((v & rm.L4_BAD_CSUM) != 0)), proto
    assert np.any(checked & (hlen > 20))                                          # IPv4 with options


def run_rxv(b, mask):
    out = np.full(b.n, 0xDEADBEEF, dtype=np.uint32)
    bad = na.rx_validate_host(b.arena, b.arena.nbytes, b.off, b.ln, out, b.n, flags=rm.F_TRAILER, bad_mask=mask)
    assert na.rxv_last_launch() == "general"
    return out, bad


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rxv_host_chunks(dev, oracle, inet_oracle, layout):
    b = rxv_case(layout, oracle, inet_oracle)
    assert_composition(b, bounds("rxv"), 0)
    assert_rxv_classes(b)
    exp = b.block_exp[b.which]
    for mask in RXV_MASKS:
        want = selected_in_every_chunk(b, exp, mask)
        out, bad = run_rxv(b, mask)
        assert_words(b, out, exp, ("rxv", hex(mask)))
        assert bad == want, (hex(mask), bad, want)


# ---- the sealer ----
def txs_frames(lens):
    """A frame of each length in `lens` (every checksum field garbage): the three protocols at four
    header lengths, padded behind the datagram or not, an ip_len beyond the frame, not IPv4, a protocol
    without a checksum; random bytes where the length holds no datagram."""
    rng = np.random.default_rng(99)
    out = []
    for j, F in enumerate(lens):
        hlen, proto = (20, 24, 44, 60)[j % 4], (PROTOS + (47,))[(j // 4) % 4]
        room = F - 14 - hlen - L4MIN.get(proto, 0)
        if room < 0 and F >= 14 + 20 + 4:
            hlen, proto = 20, 1
            room = F - 14 - hlen - L4MIN[proto]
        if room >= 0:
            pad = (min(room, 3), -2)[j // 5 % 2] if j % 5 == 0 else 0   # bytes behind the datagram; ip_len beyond the frame
            fr = bytearray(raw_frame(rng, F, hlen, proto, pad=pad, df=j % 11 != 0))
            if j % 9 == 8:
                fr[12] = 0x86
            out.append(bytes(fr))
        else:
            fr = bytearray(rng.integers(0, 256, F, dtype=np.uint8).tobytes())
            if F >= 14 and j % 2:
                fr[12:14] = b"\x08\x00"
            out.append(bytes(fr))
    return out


@functools.lru_cache(maxsize=1)
def txs_case(layout, flags, oracle, inet_oracle):
    T = 4 if flags & tm.F_FCS else 0
    b = zero_batch(T, txs_frames) if layout == "Z" else tiled_batch(layout, bounds("txs"), T, 60, txs_frames)
    b.block_sealed, b.block_st, _ = tm.seal_arena(oracle, inet_oracle, b.block, b.block_off, b.block_ln, flags)
    return b


def assert_txs_classes(b, flags):
    v, F = b.block_st, b.block_ln
    hlen = np.array([(int(b.block[int(o) + 14]) & 15) * 4 if l > 14 else 0 for o, l in zip(b.block_off, F)])
    assert np.all(((v & tm.FCS_SET) != 0) == bool(flags & tm.F_FCS))
    assert np.any(((v & (tm.IPV4 | tm.RUNT)) == 0) & (F >= 14))                  # not IPv4
    if F.min() < 14:
        assert np.any((v & tm.RUNT) != 0)
    for proto in PROTOS:
        assert np.any(((v & tm.L4_CSUM_SET) != 0) & ((v >> tm.PROTO_SHIFT) & 0xFF == proto)), proto
    assert np.any(((v & tm.L4_CSUM_SET) != 0) & (hlen > 20))                     # IPv4 with options
    assert np.any(((v & tm.IP_CSUM_SET) != 0) & ((v & tm.L4_CSUM_SET) == 0))     # header checksum only
    assert np.any((v & tm.IP_BAD_LEN) != 0)
    assert np.any(b.block_sealed != b.block)


def run_txs(b, flags, mask, status=True):
    a = b.arena.copy()
    st = np.full(b.n, 0xDEADBEEF, dtype=np.uint32) if status else None
    cnt = na.tx_seal_host(a, a.nbytes, b.off, b.ln, b.n, flags=flags, count_mask=mask, status=st)
    assert na.txs_last_launch() == "general"
    return a, st, cnt


TXS_CASES = sorted([(layout, tm.F_FCS) for layout in LAYOUTS] + [("A", 0), ("D", 0), ("Z", 0)])


@pytest.mark.parametrize("layout,flags", TXS_CASES)
def test_txs_host_chunks(dev, oracle, inet_oracle, layout, flags):
    T = 4 if flags & tm.F_FCS else 0
    b = txs_case(layout, flags, oracle, inet_oracle)
    assert_composition(b, bounds("txs"), T)
    assert_txs_classes(b, flags)
    if T == 0 and layout == "A":   # packed tight: a byte written behind a frame is the next frame's first
        assert np.array_equal(b.block_off[1:], (b.block_off + b.block_ln)[:-1])
    # frames and their FCS places never overlap: every byte has one writer
    order = np.argsort(b.off, kind="stable")
    ends = (b.off + b.ln + np.uint64(T))[order]
    assert layout == "Z" or np.all(ends[:-1] <= b.off[order][1:])
    exp_a, exp_s = b.tiled(b.block_sealed), b.block_st[b.which]
    want = selected_in_every_chunk(b, exp_s, TXS_MASK)
    a, st, cnt = run_txs(b, flags, TXS_MASK)
    assert_words(b, st, exp_s, ("txs status", flags))
    assert_arena(b, a, exp_a, ("txs arena", flags))
    assert cnt == want, (cnt, want)
    a, _, cnt = run_txs(b, flags, TXS_MASK, status=False)
    assert_arena(b, a, exp_a, ("txs arena, status = NULL", flags))
    assert cnt == want, (cnt, want)


# ---- the error return in mid-pipeline ----
def two_chunk_call(engine, oracle, inet_oracle):
    """An ordinary two-chunk call (slot 0, then slot 1), checked: no slot was left live."""
    if engine == "inet":
        b = tiled_batch("A2", bounds("inet"), 0, 120)
        assert_composition(b, bounds("inet"), 0)
        assert_words(b, run_inet(b, "ip"), oracle_batch(inet_oracle, "ip", b.arena, b.off, b.ln, None), "inet after the error")
    elif engine == "rxv":
        b = tiled_batch("A2", bounds("rxv"), 0, 60, rxv_frames)
        assert_composition(b, bounds("rxv"), 0)
        exp = rm.verdicts(oracle, inet_oracle, b.block, b.block_off, b.block_ln, rm.F_TRAILER)[b.which]
        out, bad = run_rxv(b, rm.FCS_BAD)
        assert_words(b, out, exp, "rxv after the error")
        assert bad == int(np.count_nonzero(exp & np.uint32(rm.FCS_BAD)))
    else:
        b = tiled_batch("A2", bounds("txs"), 4, 60, txs_frames)
        assert_composition(b, bounds("txs"), 4)
        sealed, st_block, _ = tm.seal_arena(oracle, inet_oracle, b.block, b.block_off, b.block_ln, tm.F_FCS)
        a, st, cnt = run_txs(b, tm.F_FCS, TXS_MASK)
        assert_words(b, st, st_block[b.which], "txs after the error")
        assert_arena(b, a, b.tiled(sealed), "txs after the error")
        assert cnt == int(np.count_nonzero(st_block[b.which] & np.uint32(TXS_MASK)))


@pytest.mark.parametrize("at", [100, 0])
@pytest.mark.parametrize("engine", hc.ENGINES)
def test_a_frame_longer_than_a_chunk_is_refused_in_mid_pipeline(dev, oracle, inet_oracle, engine, at):
    """Small frames, one frame that alone exceeds the chunk, more small frames: with the long frame
    at index 100 the first chunk is in flight when the engine refuses; nothing of it may be drained."""
    K = bounds(engine)
    T = 4 if engine == "txs" else 0
    big = K - T + 1
    small = {"inet": lambda k: [b"\x45" + bytes(59)] * k, "rxv": lambda k: rt.mixed_fixed(60, k, True, seed=4),
             "txs": lambda k: txs_frames([60] * k)}[engine](100 + at)
    lens = [60] * at + [big] + [60] * 100
    off = np.concatenate([[0], np.cumsum(np.array(lens, dtype=np.int64) + T + 3)[:-1]]).astype(np.uint64) + np.uint64(5)
    ln = np.array(lens, dtype=np.uint32)
    n = len(lens)
    arena = np.zeros(int(off[-1]) + 60 + T + 8, dtype=np.uint8)   # the long frame's pages are never touched
    for j, f in zip([j for j in range(n) if j != at], small):
        arena[int(off[j]):int(off[j]) + 60] = np.frombuffer(f, dtype=np.uint8)
    assert [c[:3] for c in hc.host_chunks(off[:at], ln[:at], K, P, T)] == ([(0, 100, "end")] if at else [])
    with pytest.raises(hc.FrameTooLong) as model:
        hc.host_chunks(off, ln, K, P, T)
    assert model.value.index == at
    before = {j: arena[int(off[j]):int(off[j]) + 64].copy() for j in range(n) if j != at}
    with pytest.raises(na.FcsError) as err:
        if engine == "inet":
            res = np.full(n, 0xA5A5, dtype=np.uint16)
            na.inet_batch_host("ip", arena, arena.nbytes, off, ln, None, res, n)
        elif engine == "rxv":
            res = np.full(n, 0xDEADBEEF, dtype=np.uint32)
            na.rx_validate_host(arena, arena.nbytes, off, ln, res, n)
        else:
            res = np.full(n, 0xDEADBEEF, dtype=np.uint32)
            na.tx_seal_host(arena, arena.nbytes, off, ln, n, flags=tm.F_FCS, status=res)
    text = str(err.value)
    assert f"{'packet' if engine == 'inet' else 'frame'} {at} of {big} bytes exceeds the {K}-byte host chunk" in text, text
    assert "EINVAL" in text
    assert np.all(res == res.dtype.type(0xA5A5 if engine == "inet" else 0xDEADBEEF))   # the launched chunk was not drained
    for j, was in before.items():                                                   # nor patched into the frames
        assert np.array_equal(arena[int(off[j]):int(off[j]) + 64], was), j
    assert not arena[int(off[at]):int(off[at]) + big + T].any()
    two_chunk_call(engine, oracle, inet_oracle)


# ---- the host forms' argument errors ----
@pytest.mark.parametrize("engine", hc.ENGINES)
def test_host_form_argument_errors(dev, oracle, inet_oracle, engine):
    keep = np.random.default_rng(8).integers(0, 256, 512, dtype=np.uint8)
    for j, f in enumerate(txs_frames([60] * 4)):
        keep[100 * j:100 * j + 60] = np.frombuffer(f, dtype=np.uint8)
    arena = keep.copy()
    word = "packet" if engine == "inet" else "frame"
    canary = np.uint16(0xA5A5) if engine == "inet" else np.uint32(0xDEADBEEF)

    def call(off, ln, out, flags=tm.F_FCS, a=None, n=None):
        a = arena if a is None else a
        off = None if off is None else np.asarray(off, dtype=np.uint64)
        ln = None if ln is None else np.asarray(ln, dtype=np.uint32)
        n = len(off) if n is None else n
        if engine == "inet":
            return na.inet_batch_host("ip", a, 512, off, ln, None, out, n)
        if engine == "rxv":
            return na.rx_validate_host(a, 512, off, ln, out, n)
        return na.tx_seal_host(a, 512, off, ln, n, flags=flags, status=out)

    def refused(off, ln, text, out=True, **kw):
        res = np.full(3, canary) if out is True else out
        with pytest.raises(na.FcsError) as err:
            call(off, ln, res, **kw)
        assert "EINVAL" in str(err.value) and text in str(err.value), str(err.value)
        assert res is None or np.all(res == canary)
        assert np.array_equal(arena, keep)   # refused before anything ran

    # a frame that starts behind the arena's end, even an empty one; one that ends a byte behind it
    refused([0, 513, 100], [60, 0, 60], f"{word} 1 [513, +0) outside the 512-byte arena")
    refused([0, 100, 400], [60, 60, 113], f"{word} 2 [400, +113) outside the 512-byte arena")
    refused([0, 100, 1 << 40], [60, 60, 1], f"{word} 2 [{1 << 40}, +1) outside the 512-byte arena")
    res = np.full(4, canary)
    if engine != "txs":   # ending with the arena, and an empty frame at its end, are fine
        end_off, end_ln = np.array([0, 100, 400, 512], dtype=np.uint64), np.array([60, 60, 112, 0], dtype=np.uint32)
        call(end_off, end_ln, res)
        want = oracle_batch(inet_oracle, "ip", arena, end_off, end_ln, None) if engine == "inet" else \
            rm.verdicts(oracle, inet_oracle, arena, end_off, end_ln, rm.F_TRAILER)
        assert np.array_equal(res, want)
    else:                 # the FCS place a byte behind the arena: refused with TXS_F_FCS, fine without it
        refused([0, 100, 400], [60, 60, 109], "FCS place of frame 2 [509, +4) outside the 512-byte arena")
        refused([0, 100, 400], [60, 60, 112], "FCS place of frame 2 [512, +4) outside the 512-byte arena")
        refused([0, 100, 512], [60, 60, 0], "FCS place of frame 2 [512, +4) outside the 512-byte arena")
        for flags, end_off, end_ln in ((tm.F_FCS, [0, 100, 300, 400], [60, 60, 60, 108]),   # the last FCS place ends with the arena
                                       (0, [0, 100, 400, 512], [60, 60, 112, 0])):
            end_off, end_ln = np.array(end_off, dtype=np.uint64), np.array(end_ln, dtype=np.uint32)
            a, res = keep.copy(), np.full(4, canary)
            assert call(end_off, end_ln, res, flags=flags, a=a) == 0
            want_a, want_s, _ = tm.seal_arena(oracle, inet_oracle, keep, end_off, end_ln, flags)
            assert np.array_equal(a, want_a) and np.array_equal(res, want_s) and not np.array_equal(a, keep)
    # null arrays with frames to do
    good = ([0, 100, 200], [60, 60, 60])
    if engine == "txs":   # the status array is optional
        assert call(*good, None, a=keep.copy()) == 0
    else:
        refused(*good, "null verdict array" if engine == "rxv" else "null pointer", out=None)
    refused(None, good[1], "null pointer", n=3)
    refused(good[0], None, "null pointer", n=3)
    with pytest.raises(na.FcsError) as err:
        call(*good, np.full(3, canary), a=0)
    assert "null pointer" in str(err.value)
    # no frames: nothing is looked at
    assert not call(None, None, None, a=0, n=0)
    assert np.array_equal(arena, keep)
