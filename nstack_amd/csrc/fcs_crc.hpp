// fcs_crc.hpp — device helpers of the CRC kernels shared by fcs_kernel.hip and the frame-walk
// kernels (rxv_kernel.hip, txs_kernel.hip, txf_kernel.hip): table staging, the slice-by-4 step, the
// shift tables' readers, a chunk's two chains and INV start, the LDS-DMA lane constants and window
// chains, the 16-lane XOR and the per-wave failing-frame counters. Device code only (included by
// the .hip translation units).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcs_launch.hpp"
#include "fcs_tables.hpp"
#include "row_work.hpp"

namespace fcs {

using row::u32x4a4;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// Frame slots (quarter-waves) per workgroup of NT threads; LDS (150 KiB) -> 1 WG per CU.
template <int NT> constexpr int kSlotsPerWg = NT / kGroup;

constexpr int kSingleMaskWords = kSingleMaxLead / 4;   // SINGLE variant: front-lane masks for words < 8
#ifndef FCS_CHAINS
#define FCS_CHAINS 2                               // independent chains per lane (2 or 4)
#endif

using row::gload;   // loads through address space 1 (global), row_work.hpp

// a ^ b ^ c in one VALU op: gfx950's v_bitop3_b32 with truth table 0x96.
__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// Clears the low t bits of w, t clamped to 0..32 (bytes of a window before the frame start). The
// clamp is one v_med3_i32: written as min/max the compiler proves t >= 0 after the max, turns the
// min unsigned and keeps two instructions.
__device__ __forceinline__ uint32_t clear_low_bits(uint32_t w, int t) {
#ifdef FCS_MASK_MINMAX   // measurement-only: the two-instruction clamp
    t = t < 0 ? 0 : (t > 32 ? 32 : t);
#else
    asm("v_med3_i32 %0, %1, 0, 32" : "=v"(t) : "v"(t));
#endif
    return w & (uint32_t)(0xFFFFFFFFull << t);
}

__device__ __forceinline__ uint32_t lds_rd(const uint8_t *lds, uint32_t byte_addr) {
    return *reinterpret_cast<const uint32_t *>(lds + byte_addr);
}

// Per-lane table bases for step4: 32 replicas (replica = lane & 31), base0 = r*4 (T3 at +0, T2 at
// +128), base1 = 0x10000 | r*4 (T1, T0).
__device__ __forceinline__ void table_bases(int lane, uint32_t &base0, uint32_t &base1) {
    const uint32_t r4 = (uint32_t)(lane & 31) * 4u;
    base0 = r4;
    base1 = 0x10000u | r4;
}

// One 4-byte step with the next word folded in: returns A_4(x) ^ wn, where
// A_4(x) = T3[x.b0] ^ T2[x.b1] ^ T1[x.b2] ^ T0[x.b3] -> 4 v_perm + 4 ds_read + 2 v_bitop3.
// base0 = r*4 (half 0: T3 at +0, T2 at +128), base1 = 0x10000 | r*4 (half 1: T1, T0).
__device__ __forceinline__ uint32_t step4(const uint8_t *lds, uint32_t x, uint32_t wn, uint32_t base0,
                                          uint32_t base1) {
    const uint32_t a0 = __builtin_amdgcn_perm(x, base0, 0x0C020400u);
    const uint32_t a1 = __builtin_amdgcn_perm(x, base0, 0x0C020500u);
    const uint32_t a2 = __builtin_amdgcn_perm(x, base1, 0x0C020600u);
    const uint32_t a3 = __builtin_amdgcn_perm(x, base1, 0x0C020700u);
#if defined(FCS_ABL_NOLDS)   // measurement-only build: LDS reads replaced by cheap VALU
    return xor3(a0 ^ (a1 >> 3), (a2 << 5) ^ (a3 >> 1), wn);
#else
    const uint32_t t3 = lds_rd(lds, a0);
    const uint32_t t2 = lds_rd(lds, a1 + 128);
    const uint32_t t1 = lds_rd(lds, a2);
    const uint32_t t0 = lds_rd(lds, a3 + 128);
    return xor3(xor3(t3, t2, t1), t0, wn);
#endif
}

// XOR of 8 table values and one extra input: 4 v_bitop3.
__device__ __forceinline__ uint32_t xor9(const uint32_t (&r)[8], uint32_t extra) {
    return xor3(xor3(r[0], r[1], r[2]), xor3(r[3], r[4], r[5]), xor3(r[6], r[7], extra));
}

// A_{96 j}(s): this lane's own nibble tables (entry e of table t at kLdsLane + t*2048 + e*128 +
// (lane & 31)*4; the slot holds the table of lane & 15).
__device__ __forceinline__ uint32_t lane_shift(const uint8_t *lds, uint32_t s, uint32_t lanebase) {
    uint32_t r[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint32_t sh = (4 * t >= 7) ? (s >> (4 * t - 7)) : (s << (7 - 4 * t));
        r[t] = lds_rd(lds, ((sh & 0x780u) | lanebase) + t * 2048);
    }
    return xor9(r, 0u);
}

// A_n(s) for one n shared by all lanes (J = A_1536, H48 = A_48, H24 = A_24):
// entry e of nibble table t at REGION + t*64 + e*4; 16 entries span 16 banks -> conflict free.
// Returns A_n(s) ^ extra.
template <uint32_t REGION>
__device__ __forceinline__ uint32_t uniform_shift(const uint8_t *lds, uint32_t s, uint32_t extra) {
    uint32_t r[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint32_t sh = (4 * t >= 2) ? (s >> (4 * t - 2)) : (s << 2);
        r[t] = lds_rd(lds, ((sh & 0x3Cu) | REGION) + t * 64);
    }
    return xor9(r, extra);
}

// Two independent 12-word chains over a chunk, merged with A_48 (fcs_kernel.hip's chunk_value
// without its measurement switches): the chunk's CRC register from start value x0.
__device__ __forceinline__ uint32_t chunk_crc(const uint8_t *lds, const uint32_t (&w)[kChunkWords], uint32_t x0,
                                              uint32_t tb0, uint32_t tb1) {
    uint32_t xa = x0 ^ w[0], xb = w[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        xa = step4(lds, xa, i < 11 ? w[i + 1] : 0u, tb0, tb1);
        xb = step4(lds, xb, i < 11 ? w[13 + i] : 0u, tb0, tb1);
    }
    return uniform_shift<kLdsH48>(lds, xa, xb);
}

// The INV start of a frame's first chunk: zr bytes from chunk start to frame start; 0 for a lane
// whose chunk does not hold the frame start.
__device__ __forceinline__ uint32_t inv_start(const uint8_t *lds, int zr) {
    const int zi = zr < 0 ? 0 : (zr > kChunkBytes - 1 ? kChunkBytes - 1 : zr);
    const uint32_t iv = lds_rd(lds, kLdsInv + 4u * (uint32_t)zi);
    return (zr >= 0 && zr < kChunkBytes) ? iv : 0u;
}

// XOR over each 16-lane row (one frame); every lane of the row ends with the row's XOR.
__device__ __forceinline__ uint32_t row_xor(uint32_t v) {
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad [1,0,3,2]
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad [2,3,0,1]
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror
    return v;
}

// CRC residue: ether_fcs(frame || LE32(ether_fcs(frame))) for every frame.
constexpr uint32_t kResidue = 0x2144DF1Cu;

template <uint32_t BAD = kLdsBad>
__device__ __forceinline__ uint64_t *wave_bad(const uint8_t *lds) {   // the kernels' own __shared__ array
    return reinterpret_cast<uint64_t *>(const_cast<uint8_t *>(lds) + BAD) + (threadIdx.x >> 6);
}

template <uint32_t BAD = kLdsBad>
__device__ __forceinline__ void init_bad(const uint8_t *lds) {
    if ((threadIdx.x & 63) == 0) *wave_bad<BAD>(lds) = 0;
}

// Chunk loads are issued at raised wave priority: a wave about to feed the memory pipe goes ahead
// of waves busy with CRC arithmetic (+1.6 % on 64 M x 1518, tools/ab.py). Scoped: the wave drops
// back to priority 0 right after its loads are issued.
#ifndef FCS_LOAD_PRIO
#define FCS_LOAD_PRIO 1
#endif
struct LoadPriority {
    __device__ __forceinline__ LoadPriority() { __builtin_amdgcn_s_setprio(FCS_LOAD_PRIO); }
    __device__ __forceinline__ ~LoadPriority() { __builtin_amdgcn_s_setprio(0); }
};

// Undo the window move of issue_chunk: true dword q = loaded dword q - dlead (q >= dlead); dwords
// q < dlead lie before the arena start, hence before the frame start, and get masked anyway.
template <int N>
__device__ __forceinline__ void shift_up(uint32_t (&d)[N], int dlead) {
#pragma unroll
    for (int b = 16; b >= 1; b >>= 1) {
        const bool take = (dlead & b) != 0;
#pragma unroll
        for (int q = N - 1; q >= 0; q--) d[q] = take ? (q >= b ? d[q - b] : 0u) : d[q];
    }
}

// Stage the constant tables into LDS (once per workgroup; grids are persistent).
template <int NT>
__device__ __forceinline__ void stage_tables(const KParams &p, uint8_t *lds) {
    const int tid = threadIdx.x;
    // data: 8192 x 16 B; each b128 store = 4 replicas of one entry
    for (int i = tid; i < 8192; i += NT) {
        const int h = i >> 12;            // 64 KiB half
        const int b = (i >> 4) & 255;     // entry
        const int odd = (i >> 3) & 1;     // +128 slot
        // half 0: T3 (+0), T2 (+128); half 1: T1 (+0), T0 (+128)
        const int k = h == 0 ? (odd ? 2 : 3) : (odd ? 0 : 1);
        const uint32_t v = p.blob[kBlobSlice + 256 * k + b];
        u32x4 vv = {v, v, v, v};
        *reinterpret_cast<u32x4 *>(lds + kLdsData + (uint32_t)i * 16) = vv;
    }
    const uint32_t *src = p.blob + kBlobLane;
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds + kLdsLane);
    for (int i = tid; i < (int)(kBlobFlat - kBlobLane); i += NT) dst[i] = src[i];
    __syncthreads();
}
// ---- LDS-DMA kernels (fcs_dma_kernel and its kin, rxv_dma_kernel): LDS layout, lookups, slot DMA ----
#ifndef FCS_DMA_CHAINS   // independent chains per lane window (2, 3, 4 or 6; measurement override)
#define FCS_DMA_CHAINS 2
#endif
constexpr int kDmaChains = FCS_DMA_CHAINS;
constexpr int kDmaChainWords = kChunkWords / kDmaChains;
static_assert(kChunkWords % kDmaChains == 0 && kDmaChainWords % 2 == 0, "chains of an even word count");
constexpr uint32_t kDmaHole = 128;                                  // byte offset of a row's hole
__host__ __device__ constexpr uint32_t dma_hole(uint32_t q) { return q * 256u + kDmaHole; }
constexpr uint32_t kDmaMergeHole = 128;                             // 4 holes per merge table
constexpr uint32_t kDmaInvHole = kDmaMergeHole + 4 * 5;             // 3 holes: INV[0..95]
constexpr uint32_t kDmaBad = dma_hole(kDmaInvHole + 3);            // 16 x 8 B
constexpr uint32_t kDmaRing = 65536;                                // slots start after the tables
constexpr int kDmaWaves = kDmaWgThreads / 64;
constexpr uint32_t kDmaLdsBytes = kDmaRing + (uint32_t)kDmaWaves * kDmaItemBytes;
static_assert(kDmaLdsBytes <= 163840, "LDS per CU");
static_assert(kDmaChains - 1 <= 5, "merge holes");
#ifndef FCS_DMA_AUX   // cache policy of the slot DMA (2 = nt; measurement-only override)
#define FCS_DMA_AUX 2
#endif
#ifndef FCS_DMA_DYN_PCT   // share of the items handed out dynamically when p.ctr is set
#define FCS_DMA_DYN_PCT 100
#endif
#ifndef FCS_DMA_CHUNK_MAX   // largest dynamic chunk (items); measurement-only override
#define FCS_DMA_CHUNK_MAX 64
#endif

// One slice-by-4 step against the 32 KiB slice tables: T_{3-s}[e] at e * 256 + s * 32 + replica * 4
// (replica = lane & 7). ds_read_b32 banks are the dword address mod 32, so the 4 slots x 8
// replicas of a row are the 32 banks. Lane group h = (lane >> 3) & 3 looks byte k ^ h up in slot
// k ^ h at its k-th lookup, so the four 8-lane groups of a 32-lane access use four different
// slots and every lookup hits 32 distinct banks. Byte and slot are per-lane constants of the
// v_perm that forms the address: selector SEL[k] picks byte k ^ h of x, base B[k] = replica * 4 +
// 32 * (k ^ h).
__device__ __forceinline__ uint32_t step4_l8(const uint8_t *lds, uint32_t x, uint32_t wn, const uint32_t (&B)[4],
                                             const uint32_t (&SEL)[4]) {
#ifdef FCS_DMA_ABL_NOLDS   // measurement-only: lookups replaced by VALU on the addresses (wrong FCS)
    const uint32_t a0 = __builtin_amdgcn_perm(x, B[0], SEL[0]), a1 = __builtin_amdgcn_perm(x, B[1], SEL[1]);
    const uint32_t a2 = __builtin_amdgcn_perm(x, B[2], SEL[2]), a3 = __builtin_amdgcn_perm(x, B[3], SEL[3]);
    return xor3(xor3(a0, a1 << 3, a2 >> 1), a3 << 7, wn);
#else
    const uint32_t t3 = lds_rd(lds, __builtin_amdgcn_perm(x, B[0], SEL[0]));
    const uint32_t t2 = lds_rd(lds, __builtin_amdgcn_perm(x, B[1], SEL[1]));
    const uint32_t t1 = lds_rd(lds, __builtin_amdgcn_perm(x, B[2], SEL[2]));
    const uint32_t t0 = lds_rd(lds, __builtin_amdgcn_perm(x, B[3], SEL[3]));
    return xor3(xor3(t3, t2, t1), t0, wn);
#endif
}

// A_{e_c}(s) from the lane tables in the holes: nibble n of table t at hole 16 t + n, slot lane & 31.
__device__ __forceinline__ uint32_t lane_shift_dma(const uint8_t *lds, uint32_t s, uint32_t lanebase) {
    uint32_t r[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint32_t sh = (4 * t >= 8) ? (s >> (4 * t - 8)) : (s << (8 - 4 * t));
        r[t] = lds_rd(lds, ((sh & 0xF00u) | lanebase) + (uint32_t)t * 4096u);
    }
    return xor9(r, 0u);
}

// Merge table m (A_{4 CL (m + 1)}): nibble table t at hole kDmaMergeHole + 4 m + t / 2, +64 (t odd).
__device__ __forceinline__ uint32_t merge_shift_dma(const uint8_t *lds, int m, uint32_t s, uint32_t extra) {
    uint32_t r[8];
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint32_t sh = (4 * t >= 2) ? (s >> (4 * t - 2)) : (s << 2);
        const uint32_t base = dma_hole(kDmaMergeHole + 4u * (uint32_t)m + (uint32_t)(t >> 1)) + 64u * (uint32_t)(t & 1);
        r[t] = lds_rd(lds, (sh & 0x3Cu) | base);
    }
    return xor9(r, extra);
}

// The per-lane constants of the LDS-DMA lookups, formed from a lane number (rxv_dma_kernel forms
// them once, txs_dma_kernel per item from an opaque lane number: DESIGN.md §3.10 "Registers").
struct DmaLane {
    uint32_t B[4], SEL[4];   // step4_l8's bases and selectors
    uint32_t lanebase;       // lane_shift_dma's
};

__device__ __forceinline__ DmaLane dma_lane(uint32_t ln) {
    const uint32_t h = (ln >> 3) & 3u, r4 = (ln & 7u) * 4u;
    return DmaLane{{r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)},
                   {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8), 0x0C0C0400u + ((2u ^ h) << 8),
                    0x0C0C0400u + ((3u ^ h) << 8)},
                   kDmaHole + (ln & 31u) * 4u};
}

// The INV start of a frame's front lane (15 of its row), whose window has zc leading bytes; 0 for the others.
__device__ __forceinline__ uint32_t dma_inv_start(const uint8_t *lds, uint32_t ln, int zc) {
    return (ln & 15u) == (uint32_t)(kGroup - 1)
               ? lds_rd(lds, dma_hole(kDmaInvHole + (uint32_t)zc / 32u) + (uint32_t)(zc % 32) * 4u)
               : 0u;
}

// kDmaChains independent chains over a lane window, merged, shifted to the frame end by the lane's
// own table: the lane's share of the frame's CRC register (row_xor joins them).
__device__ __forceinline__ uint32_t dma_chunk_crc(const uint8_t *lds, const uint32_t (&w)[kChunkWords], uint32_t x0,
                                                  const uint32_t (&B)[4], const uint32_t (&SEL)[4], uint32_t lanebase) {
    constexpr int CL = kDmaChainWords;
    uint32_t xs[kDmaChains];
#pragma unroll
    for (int hh = 0; hh < kDmaChains; hh++) xs[hh] = w[hh * CL] ^ (hh == 0 ? x0 : 0u);
#pragma unroll
    for (int i = 0; i < CL; i++)
#pragma unroll
        for (int hh = 0; hh < kDmaChains; hh++)
            xs[hh] = step4_l8(lds, xs[hh], i < CL - 1 ? w[hh * CL + i + 1] : 0u, B, SEL);
    uint32_t mv = xs[kDmaChains - 1];
#pragma unroll
    for (int hh = 0; hh < kDmaChains - 1; hh++) mv = merge_shift_dma(lds, kDmaChains - 2 - hh, xs[hh], mv);
    return lane_shift_dma(lds, mv, lanebase);
}

// The slot DMA: six 1 KiB rows from two address registers. The instruction's offset (13-bit,
// 0 .. 3 KiB here) applies to the global AND the LDS address, so each group of rows passes the
// same LDS base (one M0 value).
// The first and last row of an item share their 128-B lines with the neighbouring items: those
// two rows keep the default cache policy (the line stays in L2 for the neighbour), the middle
// rows are non-temporal; the last row is trimmed to the lanes the item's bytes reach. Both +1.1 %
// on 64 M x 1518 B (tools/ab.py).
#ifndef FCS_DMA_EDGE_AUX   // measurement-only override
#define FCS_DMA_EDGE_AUX 0
#endif
// TRIM_ALL (segmented kernel, whose items can be shorter than 5 KiB): every row only as far as
// the item's bytes reach.
template <bool TRIM_ALL = false>
__device__ __forceinline__ void dma_item(const uint8_t *slot, uint64_t src, int lane, uint32_t need) {
    typedef __attribute__((address_space(3))) void lds_void;
    static_assert(kDmaItemBytes == 6 * 1024, "six rows");
    const uint64_t a = src + 16 * (uint64_t)lane, b = a + 4096;
    lds_void *la = (lds_void *)slot, *lb = (lds_void *)(slot + 4096);
    const uint32_t o = 16u * (uint32_t)lane;
    if (!TRIM_ALL || o < need)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 0, FCS_DMA_EDGE_AUX);
    if (!TRIM_ALL || 1024u + o < need)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 1024, FCS_DMA_AUX);
    if (!TRIM_ALL || 2048u + o < need)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 2048, FCS_DMA_AUX);
    if (!TRIM_ALL || 3072u + o < need)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 3072, FCS_DMA_AUX);
    if (!TRIM_ALL || 4096u + o < need)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 0, FCS_DMA_AUX);
#ifndef FCS_DMA_NO_TRIM   // measurement-only: FCS_DMA_NO_TRIM loads the whole last row
    if (5120u + o < need)
#endif
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 1024, FCS_DMA_EDGE_AUX);
    (void)need;
}

// Table image of the LDS-DMA kernels: slice tables (16-B stores of one value: 4 replicas), lane
// tables, merge tables, INV.
template <int NT = kDmaWgThreads>
__device__ __forceinline__ void stage_dma_tables(const KParams &p, uint8_t *lds, int tid) {
    for (int i = tid; i < 2048; i += NT) {   // row e = i >> 3; store j = i & 7 -> slot j >> 1
        const uint32_t v = p.blob[kBlobSlice + 256 * (3 - ((i & 7) >> 1)) + (i >> 3)];
        u32x4 vv = {v, v, v, v};
        *reinterpret_cast<u32x4 *>(lds + (uint32_t)(i >> 3) * 256u + (uint32_t)(i & 7) * 16u) = vv;
    }
    for (int i = tid; i < 4096; i += NT)   // [t][n][slot]: hole 16 t + n
        *reinterpret_cast<uint32_t *>(lds + dma_hole((uint32_t)i >> 5) + (uint32_t)(i & 31) * 4u) = p.blob[kBlobLaneDma + i];
    for (int i = tid; i < 128 * (kDmaChains - 1); i += NT) {   // merge table m = A_{4 CL (m + 1)}
        const int m = i >> 7, t = (i >> 4) & 7, e = i & 15;
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kDmaMergeHole + 4u * (uint32_t)m + (uint32_t)(t >> 1)) +
                                      64u * (uint32_t)(t & 1) + 4u * (uint32_t)e) =
            p.blob[kBlobMerge + ((m + 1) * (kDmaChainWords / 2) - 1) * 128 + (i & 127)];
    }
    for (int i = tid; i < kChunkBytes; i += NT)
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kDmaInvHole + (uint32_t)i / 32u) + (uint32_t)(i % 32) * 4u) =
            p.blob[kBlobInv + i];
}

}  // namespace fcs
