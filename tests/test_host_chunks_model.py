"""CPU check of tests/host_chunks.py: the vectorised chunker equals the literal transcription of the
engines' chunker on a few thousand random layouts at small bounds, the transcription equals the
chunker itself (nstack_amd/csrc/host_chunk.hpp, run stand-alone under the sanitizers by
tests/c/host_chunk_check.cpp) on the same layouts, and the three engines' constants are the ones the
layouts of tests/test_gpu_host_chunks.py were sized for."""
import os
import subprocess

import numpy as np
import pytest

import host_chunks as hc

K, P = 4096, 64
KINDS = ("packed", "gapped", "shuffled", "descending", "zeros", "long")


def layout(kind, rng, T):
    """off[], len[] of one random layout (frames never overlap, every frame with T bytes behind it)."""
    n = int(rng.integers(1, 300))
    top = int(rng.choice([40, 200, 1500, K - T]))
    ln = rng.integers(0, top + 1, n)
    if kind == "zeros":
        ln[rng.random(n) < 0.6] = 0
    gap = np.zeros(n, dtype=np.int64)
    if kind == "gapped":      # around the span rule's factor 2: gaps from half to twice the frame
        gap = (ln * rng.uniform(0.5, 2.0)).astype(np.int64) + rng.integers(0, 8, n)
    elif kind != "packed":
        gap = rng.integers(0, 3, n) * rng.integers(0, 400, n)
    if kind == "long":
        ln[int(rng.integers(0, n))] = K - T + int(rng.integers(1, 50))
    slot = ln + T + gap
    off = int(rng.integers(0, 64)) + np.concatenate([[0], np.cumsum(slot)[:-1]])
    if kind == "shuffled":
        p = rng.permutation(n)
        off, ln = off[p], ln[p]
    elif kind == "descending":
        off, ln = off[::-1], ln[::-1]
    return off.astype(np.uint64), ln.astype(np.uint32)


@pytest.mark.parametrize("T", [0, 4])
def test_vectorised_chunker_equals_the_transcribed_loop(T):
    rng = np.random.default_rng(2024 + T)
    seen, refused = set(), 0
    for t in range(1800):
        kind = KINDS[t % len(KINDS)]
        off, ln = layout(kind, rng, T)
        try:
            want = hc.host_chunks_scalar(off, ln, K, P, T)
        except hc.FrameTooLong as e:
            assert kind == "long" and int(ln[e.index]) + T > K
            assert str(e) == f"frame {e.index} alone does not fit"
            with pytest.raises(hc.FrameTooLong) as got:
                hc.host_chunks(off, ln, K, P, T)
            assert got.value.index == e.index and str(got.value) == str(e)
            refused += 1
            continue
        assert kind != "long"
        assert hc.host_chunks(off, ln, K, P, T) == want, (kind, t)
        assert want[0][0] == 0 and want[-1][1] == len(off) and want[-1][2] == "end"
        assert all(a[1] == b[0] for a, b in zip(want, want[1:]))
        for i, e, bound, staging, total, span in want:
            assert 0 < e - i <= P and total <= K and total == int(ln[i:e].astype(np.int64).sum()) + T * (e - i)
            seen.add((bound, staging))
    assert refused == 1800 // len(KINDS)
    # every bound with both staging kinds ("end" included): the layouts reach the whole loop
    assert seen == {(b, s) for b in ("pkts", "bytes", "span", "end") for s in ("dense", "gather")}, seen


def test_bytes_bound_is_reported_where_the_span_rule_would_stop_too():
    # frame 2 exceeds the bytes bound and, were it taken, would trip the span rule as well
    off = np.array([0, 1600, 3200], dtype=np.uint64)
    ln = np.array([1500, 1500, 1500], dtype=np.uint32)
    for f in (hc.host_chunks, hc.host_chunks_scalar):
        assert f(off, ln, K, P, 0) == [(0, 2, "bytes", "dense", 3000, 3100), (2, 3, "end", "dense", 1500, 1500)]
    # the same frames further apart: the span rule alone refuses frame 1, then frame 2
    off = np.array([0, 3000, 6000], dtype=np.uint64)
    for f in (hc.host_chunks, hc.host_chunks_scalar):
        assert f(off, ln, K, P, 0) == [(0, 1, "span", "dense", 1500, 1500), (1, 2, "span", "dense", 1500, 1500),
                                       (2, 3, "end", "dense", 1500, 1500)]
    # and sparse (span more than twice the bytes): no cut, the chunk is gathered
    off = np.array([0, 5000, 10000], dtype=np.uint64)
    ln = np.array([1000, 1000, 1000], dtype=np.uint32)
    for f in (hc.host_chunks, hc.host_chunks_scalar):
        assert f(off, ln, K, P, 4) == [(0, 3, "end", "gather", 3012, 11004)]


# ---- the C++ chunker itself (a stand-alone program: nothing is loaded into Python) ----
HAND_MADE = (([0, 1600, 3200], [1500, 1500, 1500], 0), ([0, 3000, 6000], [1500, 1500, 1500], 0),
             ([0, 5000, 10000], [1000, 1000, 1000], 4))   # test_bytes_bound_is_reported_where_...'s three


def _layouts(T):
    """The 1800 layouts of test_vectorised_chunker_equals_the_transcribed_loop for this T, then the
    hand-made ones with this T: [(off, len)]."""
    rng = np.random.default_rng(2024 + T)
    out = [layout(KINDS[t % len(KINDS)], rng, T) for t in range(1800)]
    return out + [(np.array(o, dtype=np.uint64), np.array(l, dtype=np.uint32)) for o, l, t in HAND_MADE if t == T]


@pytest.fixture(scope="module")
def check_program():
    cdir = os.path.join(hc.ROOT, "tests", "c")
    subprocess.run(["make", "-s", "-C", cdir, "-f", "host_chunk_check.mk"], check=True)
    return os.path.join(cdir, "host_chunk_check")


@pytest.mark.parametrize("T", [0, 4])
def test_the_cxx_chunker_equals_the_transcribed_loop(check_program, T):
    lays = _layouts(T)
    text = "".join(f"{K} {P} {T} {len(off)}\n{' '.join(map(str, off))}\n{' '.join(map(str, ln))}\n" for off, ln in lays)
    r = subprocess.run([check_program], input=text, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    got = [blk.split("\n") for blk in r.stdout.split("end\n")]
    assert got.pop() == [""] and len(got) == len(lays)
    seen, refused = set(), 0
    for t, ((off, ln), lines) in enumerate(zip(lays, got)):
        assert lines.pop() == ""
        try:
            want = hc.host_chunks_scalar(off, ln, K, P, T)
        except hc.FrameTooLong as e:
            assert lines[-1] == f"toolong {e.index}", (t, lines[-1])
            refused += 1
            continue
        assert not any(x.startswith("toolong") for x in lines), t
        rows = [x.split() for x in lines]
        # (i, e, staging, sum, hi - lo) of every chunk
        assert [(int(x[0]), int(x[1]), x[5], int(x[2]), int(x[4]) - int(x[3])) for x in rows] == \
            [(i, e, staging, total, span) for i, e, _, staging, total, span in want], t
        seen |= {(bound, staging) for _, _, bound, staging, _, _ in want}
    assert refused == 1800 // len(KINDS)
    assert seen == {(b, s) for b in ("pkts", "bytes", "span", "end") for s in ("dense", "gather")}, seen


def test_engine_constants_are_the_ones_the_layouts_assume():
    assert hc.engine_constants("inet") == {"kChunkBytes": 128 << 20, "kChunkPkts": 1 << 20, "kDepth": 2}
    assert hc.engine_constants("rxv") == {"kChunkBytes": 64 << 20, "kChunkPkts": 1 << 20, "kDepth": 2}
    assert hc.engine_constants("txs") == {"kChunkBytes": 64 << 20, "kChunkPkts": 1 << 20, "kDepth": 2}
