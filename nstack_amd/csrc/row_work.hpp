// row_work.hpp — what the batch kernels whose QUARTER-WAVES (rows) each take one item at a time share
// (txf_kernel.hip, rxr_kernel.hip, dmx_kernel.hip): the global-memory accessors, the row geometry,
// and the row's run of items taken from a device work counter. Device code only
// (included by the .hip translation units).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace row {

typedef uint32_t u32x4a4 __attribute__((ext_vector_type(4), aligned(4)));

// Loads through address space 1 (global): flat loads would also count on lgkmcnt and make every
// LDS wait drain the prefetched chunk loads.
template <typename T>
__device__ __forceinline__ T gload(uint64_t addr) {
#ifdef FCS_NT   // measurement-only build: non-temporal (nt) frame loads
    return __builtin_nontemporal_load(reinterpret_cast<const __attribute__((address_space(1))) T *>(addr));
#else
    return *reinterpret_cast<const __attribute__((address_space(1))) T *>(addr);
#endif
}
template <typename T>
__device__ __forceinline__ void gstore(uint64_t addr, T v) {
    *reinterpret_cast<__attribute__((address_space(1))) T *>(addr) = v;
}

constexpr int kGroup = 16;     // lanes per row: one item (frame, datagram) at a time
constexpr uint64_t kRun = 8;   // items a row takes from the work counter at a time
constexpr int kFlight = 4;     // 16-byte pieces a lane has in flight (the copy loops of rxr_kernel and dmx_kernel)

// A row's run of consecutive items [cur, end) of a batch of n, taken from the zeroed device counter
// *ctr: one atomicAdd per wave for all its rows that ran dry, no waiting on anybody.
struct Run {
    uint64_t cur = 0, end = 0;
    // wave-uniform call: every row with `want` gets the next run
    __device__ __forceinline__ void take(bool want, unsigned long long *ctr, uint64_t n) {
        const int lane = threadIdx.x & 63, j = lane & (kGroup - 1);
        const uint64_t m = __ballot(want && j == 0);
        if (m == 0) return;
        const int leader = __ffsll((unsigned long long)m) - 1;
        unsigned long long base = 0;
        if (lane == leader) base = atomicAdd(ctr, (unsigned long long)__popcll(m) * kRun);
        base = __shfl(base, leader, 64);
        const uint64_t before = m & ((1ull << (lane & ~(kGroup - 1))) - 1ull);   // wanting rows in front of this one
        if (want) {
            cur = base + (uint64_t)__popcll(before) * kRun;
            end = cur + kRun < n ? cur + kRun : n;
        }
    }
};

// item(i) for every i < n, each by one row of the grid; the rows of a wave stay together until all
// of them are done.
template <class Item>
__device__ __forceinline__ void for_each_item(unsigned long long *ctr, uint64_t n, Item &&item) {
    Run r;
    bool done = false;
    while (true) {
        r.take(!done && r.cur >= r.end, ctr, n);
        if (!done && r.cur >= n) done = true;
        if (__all(done)) break;
        if (!done) item(r.cur++);
    }
}

}  // namespace row
