// host_chunk_check.cpp — stand-alone check of the host forms' chunker (nstack_amd/csrc/host_chunk.hpp,
// the header inet_engine.cpp, rxv_engine.cpp and txs_engine.cpp cut and stage their chunks with).
// Built with -fsanitize=address,undefined (tests/c/host_chunk_check.mk) and run by
// tests/test_host_chunks_model.py, which compares what is printed here with tests/host_chunks.py.
//
// Reads layouts from standard input, each as "K P T n", then off[0..n), then len[0..n). Per layout it
// cuts from 0 to n and prints one line per chunk, "i e sum lo hi dense|gather", or "toolong i" where
// frame i alone does not fit (the layout ends there), then "end". Every chunk is staged into a heap
// buffer of exactly K + 64 bytes and an offset array of exactly P entries, from an arena of exactly
// the bytes the frames cover, so that an overrun on either side is a sanitizer report; what was
// staged is checked against the arena. A failed check prints the chunk and returns 1.
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nstack_amd/csrc/host_chunk.hpp"

static bool staged_right(const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t i,
                         const hostchunk::Cut &c, uint64_t K, uint64_t T, const uint8_t *h_in, const uint64_t *h_off,
                         uint64_t span) {
    const bool dense = hostchunk::dense(c, K);
    uint64_t w = 0;
    for (uint64_t q = 0; q < c.e - i; q++) {
        const uint64_t o = off[i + q], l = len[i + q];
        if (h_off[q] > K + 64 || l > K + 64 - h_off[q]) return false;
        if (std::memcmp(h_in + h_off[q], arena + o, l) != 0) return false;   // each staged frame is its arena bytes
        if (dense && (h_off[q] & 15) != (o & 15)) return false;              // dense: alignment kept mod 16
        if (!dense && h_off[q] != w) return false;                           // gathered: len + T apart from 0
        w += l + T;
    }
    return span == (dense ? (c.lo & 15) + (c.hi - c.lo) : w) && w == c.sum;
}

int main() {
    uint64_t K, P, T, n;
    while (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &K, &P, &T, &n) == 4) {
        std::vector<uint64_t> off(n);
        std::vector<uint32_t> len(n);
        for (uint64_t &o : off)
            if (std::scanf("%" SCNu64, &o) != 1) return 2;
        for (uint32_t &l : len)
            if (std::scanf("%" SCNu32, &l) != 1) return 2;
        uint64_t top = 0;
        for (uint64_t q = 0; q < n; q++) top = std::max(top, off[q] + len[q] + T);
        // exactly the stated sizes, on the heap
        uint8_t *arena = (uint8_t *)std::malloc(top ? top : 1), *h_in = (uint8_t *)std::malloc(K + 64);
        uint64_t *h_off = (uint64_t *)std::malloc(P * 8);
        for (uint64_t x = 0; x < top; x++) arena[x] = (uint8_t)(x * 167 + (x >> 8) * 13 + 1);
        int bad = 0;
        for (uint64_t i = 0; i < n && !bad;) {
            const hostchunk::Cut c = hostchunk::cut(off.data(), len.data(), i, n, K, P, T);
            if (c.e == i) {
                std::printf("toolong %" PRIu64 "\n", i);
                break;
            }
            std::printf("%" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %s\n", i, c.e, c.sum, c.lo, c.hi,
                        hostchunk::dense(c, K) ? "dense" : "gather");
            std::memset(h_in, 0, K + 64);
            const uint64_t span = hostchunk::stage(arena, off.data(), len.data(), i, c, K, T, h_in, h_off,
                                                  [](uint8_t *d, const uint8_t *s, uint64_t b) { std::memcpy(d, s, b); });
            if (!staged_right(arena, off.data(), len.data(), i, c, K, T, h_in, h_off, span)) {
                std::printf("FAIL staging of the chunk above (span %" PRIu64 ")\n", span);
                bad = 1;
            }
            i = c.e;
        }
        std::free(arena);
        std::free(h_in);
        std::free(h_off);
        if (bad) return 1;
        std::printf("end\n");
    }
    return 0;
}
