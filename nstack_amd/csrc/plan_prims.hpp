// plan_prims.hpp — what the plan launches of the batch engines share (txf_kernel.hip, rxr_kernel.hip,
// gro_kernel.hip, dmx_kernel.hip). Host part: the plan kernels' workgroup size, the
// sizes of their grids and tables, and the launch chain. Device part (the .hip translation units
// only): the workgroup scan, the one-workgroup scan of the block totals, and the hash and the probe
// loop of the open-addressing tables.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace plan {

constexpr int kPlanThreads = 256;   // the plan kernels: one item per thread

inline uint64_t plan_blocks(uint64_t n) { return (n + kPlanThreads - 1) / kPlanThreads; }
// Entries of an open-addressing table that takes at most n claims: a power of two, >= 2 n, so that
// the table cannot fill and an empty entry ends every miss.
inline uint64_t table_size(uint64_t n) {
    uint64_t t = 16;
    while (t < 2 * n) t <<= 1;
    return t;
}
inline uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }

// One launch of a chain: returns the launch's own error from the enclosing launcher.
#define PLAN_LAUNCH(...)                                              \
    do {                                                              \
        hipLaunchKernelGGL(__VA_ARGS__);                              \
        const hipError_t e_ = hipGetLastError();                      \
        if (e_ != hipSuccess) return e_;                              \
    } while (0)

#ifdef __HIPCC__
// Inclusive scan over the workgroup of kPlanThreads (sh: that many T); total: the workgroup's sum.
template <class T>
__device__ __forceinline__ T block_scan_incl(T v, T *sh, T &total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < kPlanThreads; o <<= 1) {
        const T add = t >= o ? sh[t - o] : (T)0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const T r = sh[t];
    total = sh[kPlanThreads - 1];
    __syncthreads();   // sh is free for the next call
    return r;
}
template <class T>
__device__ __forceinline__ T block_scan_excl(T v, T *sh) {
    T total;
    return block_scan_incl(v, sh, total) - v;
}

// One workgroup: the nb block totals tot[] become the sums of the blocks in front. Returns the sum
// of all.
template <class T>
__device__ __forceinline__ T scan_totals(T *tot, uint64_t nb, T *sh) {
    T base = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += kPlanThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const T v = b < nb ? tot[b] : (T)0;
        T total;
        const T incl = block_scan_incl(v, sh, total);
        if (b < nb) tot[b] = base + incl - v;
        base += total;
    }
    return base;
}

// The 32-bit hash of a four-word key.
__device__ __forceinline__ uint64_t mix4(uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    uint32_t h = a * 0x9E3779B1u ^ b * 0x85EBCA77u ^ c * 0xC2B2AE3Du ^ d * 0x27D4EB2Fu;
    h ^= h >> 15;
    h *= 0x2C1B3C6Du;
    h ^= h >> 12;
    h *= 0x297A2D39u;
    h ^= h >> 15;
    return h;
}

// Linear probing from hash h in a table of tsize entries (a power of two): visit(slot) returns true
// to stop. At most tsize probes. Returns whether a visit stopped the walk.
template <class Visit>
__device__ __forceinline__ bool probe(uint64_t tsize, uint64_t h, Visit &&visit) {
    const uint64_t mask = tsize - 1;
    h &= mask;
    for (uint64_t t = 0; t < tsize; t++) {
        if (visit(h)) return true;
        h = (h + 1) & mask;
    }
    return false;
}
#endif   // __HIPCC__

}  // namespace plan
