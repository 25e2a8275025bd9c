"""The chunker of the host forms inet_csum_batch_host, ether_rx_validate_host and ether_tx_seal_host
restated: the three engines cut a batch into chunks with one C++ function (hostchunk::cut in
nstack_amd/csrc/host_chunk.hpp: the packet bound, the byte bound and the span rule) and stage each
chunk densely or gathered. `host_chunks` is the vectorised restatement the GPU tests assert their
layouts with, `host_chunks_scalar` the literal transcription of the C++ loop; tests/test_host_chunks_model.py
holds the first to the second, and the second to the C++ function itself, run stand-alone by
tests/c/host_chunk_check.cpp. Test infrastructure only."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENGINES = ("inet", "rxv", "txs")


def engine_constants(name):
    """The host pipeline's bounds, read from {inet,rxv,txs}_engine.cpp: {name: value}."""
    assert name in ENGINES, name
    with open(os.path.join(ROOT, "nstack_amd", "csrc", name + "_engine.cpp")) as f:
        src = f.read()
    k = {m[0]: int(m[1]) << int(m[2]) for m in re.findall(r"constexpr uint64_t (k\w+) = (\d+)ull << (\d+);", src)}
    k.update({m[0]: int(m[1]) for m in re.findall(r"constexpr int (k\w+) = (\d+);", src)})
    assert set(k) == {"kChunkBytes", "kChunkPkts", "kDepth"}, (name, k)
    return k


class FrameTooLong(ValueError):
    """Frame `index` alone does not fit a chunk: the engine's "exceeds the ... host chunk" return."""

    def __init__(self, index):
        super().__init__(f"frame {index} alone does not fit")
        self.index = index


def _kind(span, K):
    return "dense" if span <= K else "gather"


def host_chunks_scalar(off, ln, K, P, T):
    """The while loop of hostchunk::cut, line by line: [(i, e, bound, staging, sum, span)]."""
    off, ln = [int(x) for x in off], [int(x) for x in ln]
    n, i, out = len(off), 0, []
    while i < n:
        e, total, lo, hi, bound = i, 0, 1 << 64, 0, None
        while True:
            if not e < n:
                bound = "end"
                break
            if not e - i < P:
                bound = "pkts"
                break
            if not total + ln[e] + T <= K:
                bound = "bytes"
                break
            nlo, nhi = min(lo, off[e]), max(hi, off[e] + ln[e] + T)
            if e > i and nhi - nlo > K and nhi - nlo <= 2 * (total + ln[e] + T):
                bound = "span"
                break
            total += ln[e] + T
            lo, hi = nlo, nhi
            e += 1
        if e == i:
            raise FrameTooLong(i)
        out.append((i, e, bound, _kind(hi - lo, K), total, hi - lo))
        i = e
    return out


def host_chunks(off, ln, K, P, T):
    """The chunks the host forms make of off[] and len[]: [(i, e, bound, staging, sum, span)], frames
    [i, e); `bound` is what refused frame e ("pkts", "bytes", "span"; "bytes" where both of the last
    two would, since the loop tests it first) or "end"; `staging` is "dense" (one span copy) or
    "gather"; T = 4 for the sealer with TXS_F_FCS (every frame counts with its FCS place), else 0.
    The span rule is not monotone in e, so each chunk is the first stop in a window of P frames."""
    off = np.asarray(off).astype(np.int64)
    ln = np.asarray(ln).astype(np.int64) + T
    n, i, out = len(off), 0, []
    while i < n:
        o, l = off[i:i + P], ln[i:i + P]
        total = np.cumsum(l)
        span = np.maximum.accumulate(o + l) - np.minimum.accumulate(o)
        stop_bytes = total > K
        stop_span = (span > K) & (span <= 2 * total)
        stop_span[0] = False
        stop = stop_bytes | stop_span
        if stop.any():
            k = int(np.argmax(stop))
            bound = "bytes" if stop_bytes[k] else "span"
        elif i + P < n:
            k, bound = P, "pkts"
        else:
            k, bound = n - i, "end"
        if k == 0:
            raise FrameTooLong(i)
        out.append((i, i + k, bound, _kind(int(span[k - 1]), K), int(total[k - 1]), int(span[k - 1])))
        i += k
    return out
