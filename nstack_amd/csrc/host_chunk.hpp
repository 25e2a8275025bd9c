// host_chunk.hpp — the chunker of the host forms inet_csum_batch_host, ether_rx_validate_host and
// ether_tx_seal_host: where a batch is cut into pipeline chunks, and how a chunk's frames get into
// the pinned staging buffer. Host-only (no HIP), so that tests/c/host_chunk_check.cpp runs this very
// code on the CPU against the model in tests/host_chunks.py. The bounds are the caller's: K bytes and
// P frames per chunk; T is the bytes behind each frame that belong to it (the sealer's FCS place).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>

namespace hostchunk {

struct Cut {
    uint64_t e, sum, lo, hi;   // frames [i, e), their bytes (T included), and the arena span [lo, hi) they cover
};

// The chunk that starts at frame i: at most P frames, K frame bytes, and (so that densely packed
// frames go over as one span copy) a span of at most K unless the frames are sparse (span > 2x their
// bytes), which are gathered instead. e == i: frame i alone does not fit.
inline Cut cut(const uint64_t *off, const uint32_t *len, uint64_t i, uint64_t n, uint64_t K, uint64_t P, uint64_t T) {
    Cut c{i, 0, UINT64_MAX, 0};
    while (c.e < n && c.e - i < P && c.sum + len[c.e] + T <= K) {
        const uint64_t nlo = std::min(c.lo, off[c.e]), nhi = std::max(c.hi, off[c.e] + len[c.e] + T);
        if (c.e > i && nhi - nlo > K && nhi - nlo <= 2 * (c.sum + len[c.e] + T)) break;
        c.sum += len[c.e] + T;
        c.lo = nlo;
        c.hi = nhi;
        c.e++;
    }
    return c;
}

inline bool dense(const Cut &c, uint64_t K) { return c.hi - c.lo <= K; }

// Stages chunk [i, c.e) into h_in (K + 64 bytes) and its rebased offsets into h_off; returns the
// bytes of h_in to copy to the device. Dense: the span as one span_copy(dst, src, bytes), offsets
// rebased with their alignment kept mod 16. Sparse: gathered back to back (any start alignment is
// fine), each frame followed by its T free bytes.
template <class SpanCopy>
uint64_t stage(const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t i, const Cut &c, uint64_t K,
               uint64_t T, uint8_t *h_in, uint64_t *h_off, SpanCopy &&span_copy) {
    const uint64_t np = c.e - i;
    if (dense(c, K)) {
        const uint64_t pad = c.lo & 15;
        span_copy(h_in + pad, arena + c.lo, c.hi - c.lo);
        for (uint64_t q = 0; q < np; q++) h_off[q] = off[i + q] - c.lo + pad;
        return pad + (c.hi - c.lo);
    }
    uint64_t w = 0;
    for (uint64_t q = 0; q < np; q++) {
        std::memcpy(h_in + w, arena + off[i + q], len[i + q]);
        h_off[q] = w;
        w += len[i + q] + T;
    }
    return w;
}

}  // namespace hostchunk
