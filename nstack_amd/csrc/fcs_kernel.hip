// fcs_kernel.hip — batched Ethernet FCS (CRC-32/ISO-HDLC) for CDNA4 / gfx950 (MI355X).
//
// Replaces the per-frame byte loop of ether_fcs() (/root/reference/src/ether_fcs.c:13-16) with
// one launch over many independent frames. Result per frame is bit-identical to ether_fcs().
//
// Work decomposition:
//   * one QUARTER-WAVE (16 lanes) per frame; lane j owns the 96-byte chunk that ends 96*j bytes
//     before the frame end, so 16 lanes cover one 1536-byte "segment"; longer frames are walked
//     segment by segment, front to back (jumbo 9000 B = 6 segments); a wave works on 4 frames;
//   * each lane loads its chunk with 6 x global_load_dwordx4 + 1 dword from a 4-byte aligned
//     address (this layout streams HBM at the rate of a coalesced read: tools/microbench), two
//     chunks in flight per lane; the words are re-aligned to the frame end with v_alignbyte_b32
//     and the bytes in front of the frame start are zeroed;
//   * the lane runs its 24 words as four independent 6-word slice-by-4 chains (ILP 4): per word
//     4 ds_read_b32 from byte tables replicated 32x in LDS (replica = lane & 31 -> every 32-lane
//     LDS access is bank-conflict free), each address formed by ONE v_perm_b32; the chains are
//     merged as A_48(A_24(a) ^ b) ^ (A_24(c) ^ d) with nibble tables;
//   * the frame's all-ones initial register is injected as the front lane's start value
//     INV[z] = A_z^{-1}(~0) (z = zero bytes in front of the frame start); across segments a
//     lane accumulates S = A_1536(S) ^ segment value, so consecutive items stay independent;
//   * at the frame end lane j shifts its register by 96*j zero bytes (per-lane nibble tables,
//     bank = lane), the 16 registers are XOR-reduced with 4 DPP steps and lane 15 stores ~crc.
// No MFMA: a byte-stream codec bounded by HBM read bandwidth (roofline: DESIGN.md §4).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "dispenser.hpp"
#include "fcs_launch.hpp"
#include "fcs_tables.hpp"
#include "fcs_crc.hpp"
#include "wave_sync.hpp"

namespace fcs {

struct Item {
    uint64_t end;   // byte address one past the frame's last byte
    uint32_t len;
    uint32_t m;     // segments
};

template <bool VAR>
__device__ __forceinline__ Item frame_item(const KParams &p, uint64_t f) {
    Item it;
    if (VAR) {
        const uint32_t L = p.len[f];
        it.end = p.base + (p.off ? p.off[f] : f * p.stride) + L;
        it.len = L;
        it.m = L ? (L + (kSegBytes - 1)) / kSegBytes : 1u;
    } else {
        it.end = p.base + f * p.stride + p.flen;
        it.len = p.flen;
        it.m = p.fseg;
    }
    return it;
}

// Result store for one frame per lane with st set; called by the whole wave (convergent).
// FCS mode: out[i] = FCS. Verify mode (ok != null; frames carry their FCS trailer): ok[i] = 1 iff
// the FCS over the whole frame equals the residue; non-matching frames are counted in the wave's
// LDS slot (lane 0 only touches it) and added to *bad once per wave at kernel exit (flush_bad), so
// an all-bad batch costs no atomics on the data path. Both outputs may be requested together.
// BAD: LDS byte offset of the per-wave counters (kLdsBad; the LDS-DMA kernel keeps them elsewhere).
template <uint32_t BAD = kLdsBad>
__device__ __forceinline__ void emit(const KParams &p, const uint8_t *lds, bool st, uint64_t i, uint32_t fcs) {
    if (p.out != nullptr && st) p.out[i] = fcs;
    if (p.ok != nullptr) {
        const bool good = fcs == kResidue;
        if (st) p.ok[i] = good ? 1 : 0;
        const uint64_t m = __ballot(st && !good);
        if (m != 0 && (threadIdx.x & 63) == 0) *wave_bad<BAD>(lds) += (uint64_t)__popcll(m);
    }
}

template <uint32_t BAD = kLdsBad>
__device__ __forceinline__ void flush_bad(const KParams &p, const uint8_t *lds) {
    if (p.ok != nullptr && (threadIdx.x & 63) == 0) {
        const uint64_t b = *wave_bad<BAD>(lds);
        if (b) atomicAdd(p.bad, (unsigned long long)b);
    }
}

// Raw loads of one lane chunk (issued one item ahead of their use) and what is needed to
// interpret them. The register-load kernels' loads are unconditional and stay inside [lo4, hi4)
// (the LDS-DMA kernels read whole 16-B pieces instead: fcs_dma_kernel): lanes with nothing to load
// read lo4; a window that starts before lo4 (front lane of a frame at the very start of the
// arena) is moved up to lo4 in a wave-uniform branch and shifted back after the data has landed
// (process()).
struct Chunk {
    u32x4a4 x[6];
    uint32_t x6;
    int zr;        // bytes from chunk start to frame start (segment 0); -1 inside; 96 = no data
    uint32_t r;    // chunk start & 3 (realignment)
    int dlead;     // dwords the load window was moved up to stay >= lo4 (0 = not moved)
};

template <bool VAR, bool TINY, bool SINGLE>
__device__ __forceinline__ void issue_chunk(const KParams &p, const Item &it, uint32_t k, int j,
                                            bool act, Chunk &c) {
    LoadPriority lp;
    int64_t cstart;
    if (SINGLE) {   // fixed length, one segment: zr does not depend on the frame
        cstart = (int64_t)it.end - (int64_t)kChunkBytes * (j + 1);
        const int z = kChunkBytes * (j + 1) - (int)p.flen;
        c.zr = z < -1 ? -1 : (z > kChunkBytes ? kChunkBytes : z);
    } else {
        cstart = (int64_t)it.end - (int64_t)kSegBytes * (int64_t)(it.m - 1 - k) -
                 (int64_t)kChunkBytes * (j + 1);
        const int64_t z = (k == 0) ? ((int64_t)(it.end - it.len) - cstart) : -1;
        c.zr = z < -1 ? -1 : (z > kChunkBytes ? kChunkBytes : (int)z);
    }
    c.r = (uint32_t)cstart & 3u;
    const bool need = act && c.zr < kChunkBytes;
    const uint64_t a = need ? ((uint64_t)cstart & ~3ull) : p.lo4;
    c.dlead = 0;
    if (TINY) {
        // Arena shorter than 192 B (host-selected variant): per-dword guarded loads.
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q <= kChunkWords; q++) {
            const uint64_t ad = a + 4 * q;
            d[q] = (need && ad >= p.lo4 && ad + 4 <= p.hi4) ? gload<uint32_t>(ad) : 0u;
        }
#pragma unroll
        for (int g = 0; g < 6; g++) c.x[g] = u32x4a4{d[4 * g], d[4 * g + 1], d[4 * g + 2], d[4 * g + 3]};
        c.x6 = d[kChunkWords];
        return;
    }
    // High side in bounds by construction: a + 96 <= chunk end <= hi4; the 25th dword (needed
    // only when r != 0) ends at ceil4(chunk end) <= hi4; when r == 0 dword 23 is re-read instead.
    // Low side: a window starting before lo4 (front lane of a frame at the arena start) is moved
    // up to lo4 as a whole; process() shifts the dwords back by dlead (wave-uniform, rare branch).
    uint64_t ab = a;
    if (__any(a < p.lo4)) {
        c.dlead = a < p.lo4 ? (int)((p.lo4 - a) >> 2) : 0;
        ab = a < p.lo4 ? p.lo4 : a;
    }
#pragma unroll
    for (int q = 0; q < 6; q++) c.x[q] = gload<u32x4a4>(ab + 16 * q);
    c.x6 = gload<uint32_t>(ab + ((c.r || c.dlead) ? 96 : 92));
}

#ifndef FCS_FIXED_CHUNK_MAX   // measurement-only overrides: largest dynamic chunk, in units
#define FCS_FIXED_CHUNK_MAX 64   // generic fixed kernel: units of 4 frames
#endif
#ifndef FCS_FIXED_DYN_PCT
#define FCS_FIXED_DYN_PCT 100    // generic fixed kernel: share of the units handed out dynamically
#endif
#ifndef FCS_FLAT_CHUNK_MAX
#define FCS_FLAT_CHUNK_MAX 16    // flat kernel: 64-frame windows
#endif

template <bool VAR, bool TINY, bool SINGLE>
struct Lane {
    const KParams &p;
    const uint8_t *lds;
    int j;            // lane within the frame's 16
    uint32_t base0, base1, lanebase;
    uint64_t Q;       // frame slots in the grid
    Dispenser *D;     // fixed frames (kUnits): wave units of 4 frames; otherwise unused
    uint32_t q;       // quarter of the wave (frame 4u + q of unit u)

    struct Pos {
        uint64_t f;
        uint64_t u;   // D's unit (D only)
        uint32_t k;
        bool act;
        Item it;
    };

    static constexpr bool kUnits = !VAR && !SINGLE && !TINY;

    __device__ __forceinline__ Pos next(const Pos &c) const {
        Pos n = c;
        if (kUnits) {
            // every frame has p.fseg segments: the quarters wrap together, the unit step is uniform
            n.k = c.k + 1;
            if (n.k >= p.fseg) {
                n.k = 0;
                n.u = c.u == Dispenser::kEnd ? c.u : D->next(c.u);
                n.f = n.u == Dispenser::kEnd ? p.n : 4 * n.u + q;
            }
        } else if (SINGLE) {
            n.f = c.f + Q;
            n.k = 0;
        } else {
            n.k = c.k + 1;
            if (n.k >= c.it.m) {
                n.f = c.f + Q;
                n.k = 0;
            }
        }
        n.act = c.act && n.f < p.n;
        if (SINGLE || (n.act && n.k == 0)) n.it = frame_item<VAR>(p, n.f);
        return n;
    }

    // Consume one chunk: realign, mask, run the two chains, finish the frame if last.
    __device__ __forceinline__ void process(const Pos &c, const Chunk &ch, uint32_t &s) const {
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q < 6; q++) {
            d[4 * q] = ch.x[q].x;
            d[4 * q + 1] = ch.x[q].y;
            d[4 * q + 2] = ch.x[q].z;
            d[4 * q + 3] = ch.x[q].w;
        }
        d[kChunkWords] = ch.x6;
        if (!TINY && __any(ch.dlead)) shift_up(d, ch.dlead);   // arena start only; uniform
        uint32_t w[kChunkWords];
#pragma unroll
        for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], ch.r);
#ifdef FCS_ABL_NOCOMPUTE   // measurement-only build: loads + realign
        {
            uint32_t acc = 0;
#pragma unroll
            for (int i = 0; i < kChunkWords; i++) acc ^= w[i];
            s ^= acc;
            if (c.act && j == 15 && s == 0x12345678u) p.out[c.f] = s;
            return;
        }
#endif
        uint32_t x0 = 0;
        const bool first = SINGLE || c.k == 0;
        if (first) {
#pragma unroll
            for (int i = 0; i < kChunkWords; i++) {
                // uniform bound: words no front lane can mask are skipped. SINGLE launches only when
                // zmax <= 32 (host), so at most 8 loop-invariant masks stay live in registers.
                if ((!SINGLE || i < kSingleMaskWords) && 4 * i < (int)p.zmax) {
                    int t = ch.zr - 4 * i;
                    t = t < 0 ? 0 : (t > 4 ? 4 : t);
                    w[i] &= (uint32_t)(0xFFFFFFFFull << (8 * t));
                }
            }
            const int zi = ch.zr < 0 ? 0 : (ch.zr > kChunkBytes - 1 ? kChunkBytes - 1 : ch.zr);
            const uint32_t iv = lds_rd(lds, kLdsInv + 4u * (uint32_t)zi);
            x0 = (ch.zr >= 0 && ch.zr < kChunkBytes) ? iv : 0u;
        }
#if FCS_CHAINS == 2
        // Two independent 12-word chains, merged with A_48.
        uint32_t xa = x0 ^ w[0], xb = w[12];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            xa = step4(lds, xa, i < 11 ? w[i + 1] : 0u, base0, base1);
            xb = step4(lds, xb, i < 11 ? w[13 + i] : 0u, base0, base1);
        }
        const uint32_t r = uniform_shift<kLdsH48>(lds, xa, xb);
#else
        // Four independent 6-word chains (ILP 4 on the LDS/VALU latency), merged as a tree.
        uint32_t xa = x0 ^ w[0], xb = w[6], xc = w[12], xd = w[18];
#pragma unroll
        for (int i = 0; i < 6; i++) {
            xa = step4(lds, xa, i < 5 ? w[i + 1] : 0u, base0, base1);
            xb = step4(lds, xb, i < 5 ? w[7 + i] : 0u, base0, base1);
            xc = step4(lds, xc, i < 5 ? w[13 + i] : 0u, base0, base1);
            xd = step4(lds, xd, i < 5 ? w[19 + i] : 0u, base0, base1);
        }
        const uint32_t ab = uniform_shift<kLdsH24>(lds, xa, xb);
        const uint32_t cd = uniform_shift<kLdsH24>(lds, xc, xd);
        const uint32_t r = uniform_shift<kLdsH48>(lds, ab, cd);
#endif
        s = first ? r : uniform_shift<kLdsJump>(lds, s, r);

        const bool last = c.act && (SINGLE || c.k + 1 == c.it.m);
#ifdef FCS_ABL_NOFINAL   // measurement-only build: no lane shift / reduction
        if (last && j == 15) p.out[c.f] = s;
        return;
#endif
        if (__any(last)) {
            uint32_t v = last ? lane_shift(lds, s, lanebase) : 0u;
            v = row_xor(v);
            emit(p, lds, last && j == 15, c.f, c.it.len ? ~v : 0u);
        }
    }
};

// Flat variable-length kernel staging: the same data and uniform tables, and the chunk-shift
// tables C_c in place of the per-lane tables.
__device__ __forceinline__ void stage_tables_flat(const KParams &p, uint8_t *lds) {
    const int tid = threadIdx.x;
    for (int i = tid; i < 8192; i += kWgThreads) {
        const int h = i >> 12, b = (i >> 4) & 255, odd = (i >> 3) & 1;
        const int k = h == 0 ? (odd ? 2 : 3) : (odd ? 0 : 1);
        const uint32_t v = p.blob[kBlobSlice + 256 * k + b];
        u32x4 vv = {v, v, v, v};
        *reinterpret_cast<u32x4 *>(lds + kLdsData + (uint32_t)i * 16) = vv;
    }
    uint32_t *dst = reinterpret_cast<uint32_t *>(lds + kLdsJump);
    for (int i = tid; i < (int)(kBlobFlat - kBlobJump); i += kWgThreads) dst[i] = p.blob[kBlobJump + i];
    uint32_t *fl = reinterpret_cast<uint32_t *>(lds + kLdsFlat);
    for (int i = tid; i < (int)(kFlatBytes / 4); i += kWgThreads) fl[i] = p.blob[kBlobFlat + i];
    __syncthreads();
}

// The quarter-wave-per-frame loop of one workgroup (`blk` of `nblk`), tables already in LDS.
template <bool VAR, bool TINY, bool SINGLE, int NT>
__device__ __forceinline__ void fcs_body(const KParams &p, const uint8_t *lds, uint32_t blk, uint32_t nblk) {
    const int lane = threadIdx.x & 63;
    const int j = lane & (kGroup - 1);
    const uint32_t r4 = (uint32_t)(lane & 31) * 4u;
    uint32_t tb0, tb1;
    table_bases(lane, tb0, tb1);
    // Fixed frames: a wave's unit is 4 consecutive frames (one per quarter), units from the
    // dispenser (interleaved over the grid's waves, the tail dynamic when the host gave a counter).
    // L.D always points at D (the unit path is chosen at compile time): a pointer that could be null
    // made the compiler keep D's 120 bytes in scratch memory, loaded and stored at every unit step.
    constexpr bool kUnits = Lane<VAR, TINY, SINGLE>::kUnits;
    Dispenser D(kUnits ? p.ctr : nullptr, (p.n + 3) >> 2, (uint64_t)nblk * (NT / 64),
                (uint64_t)blk * (NT / 64) + (threadIdx.x >> 6), lane, FCS_FIXED_DYN_PCT, 1, FCS_FIXED_CHUNK_MAX);
    Lane<VAR, TINY, SINGLE> L{p, lds, j, tb0, tb1, kLdsLane | r4, (uint64_t)nblk * kSlotsPerWg<NT>,
                              &D, (uint32_t)(threadIdx.x >> 4) & 3u};

    typename Lane<VAR, TINY, SINGLE>::Pos A, B;
    if (kUnits) {
        A.u = D.first();
        A.f = A.u == Dispenser::kEnd ? p.n : 4 * A.u + L.q;
    } else {
        A.u = 0;
        A.f = ((uint64_t)blk * kSlotsPerWg<NT>) + (threadIdx.x / kGroup);
    }
    A.k = 0;
    A.act = A.f < p.n;
    A.it = (SINGLE || A.act) ? frame_item<VAR>(p, A.f) : Item{0, 0, 1};
    Chunk CA, CB;
    issue_chunk<VAR, TINY, SINGLE>(p, A.it, A.k, j, A.act, CA);
    uint32_t s = 0;

#ifndef FCS_PREFETCH_DEPTH
#define FCS_PREFETCH_DEPTH 2
#endif
#if FCS_PREFETCH_DEPTH == 2
    // Two items in flight per lane: process one while the other's loads are outstanding.
    while (__any(A.act)) {
        B = L.next(A);
        issue_chunk<VAR, TINY, SINGLE>(p, B.it, B.k, j, B.act, CB);
        L.process(A, CA, s);
        if (!__any(B.act)) break;
        A = L.next(B);
        issue_chunk<VAR, TINY, SINGLE>(p, A.it, A.k, j, A.act, CA);
        L.process(B, CB, s);
    }
#else
    // Three chunk buffers: while one item is processed the next two have their loads in flight.
    typename Lane<VAR, TINY, SINGLE>::Pos C;
    Chunk CC;
    B = L.next(A);
    issue_chunk<VAR, TINY, SINGLE>(p, B.it, B.k, j, B.act, CB);
    for (;;) {
        if (!__any(A.act)) break;
        C = L.next(B);
        issue_chunk<VAR, TINY, SINGLE>(p, C.it, C.k, j, C.act, CC);
        L.process(A, CA, s);
        if (!__any(B.act)) break;
        A = L.next(C);
        issue_chunk<VAR, TINY, SINGLE>(p, A.it, A.k, j, A.act, CA);
        L.process(B, CB, s);
        if (!__any(C.act)) break;
        B = L.next(A);
        issue_chunk<VAR, TINY, SINGLE>(p, B.it, B.k, j, B.act, CB);
        L.process(C, CC, s);
    }
#endif
}

template <bool VAR, bool TINY, bool SINGLE, int NT>
__global__ __launch_bounds__(NT, 1) void fcs_kernel(KParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    stage_tables<NT>(p, lds);
    init_bad(lds);
    fcs_body<VAR, TINY, SINGLE, NT>(p, lds, blockIdx.x, gridDim.x);
    flush_bad(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Fixed length, one segment, at most 32 leading garbage bytes in the front lane (host-selected:
// 1504 <= len <= 1536, which covers the 1518-B benchmark frames). The generic kernel's work per
// item, strength-reduced: the frame end advances by a constant, the per-lane chunk offset, front
// masks and INV start value are loop invariants, and only a wave's first item can touch the
// arena start, so the edge repair is peeled out of the loop.
// ---------------------------------------------------------------------------------------------
struct Raw {
    u32x4a4 x[6];
    uint32_t x6;
};

__device__ __forceinline__ uint64_t stamp() {
    return __builtin_amdgcn_s_memtime();
}

struct SingleLane {
    uint64_t *dbg;
    const KParams *kp;
    const uint8_t *lds;
    int j;
    uint32_t base0, base1, lanebase, x0, zmax;
    uint32_t m[kSingleMaskWords];

    template <bool EDGE>
    __device__ __forceinline__ void process(const Raw &c, uint32_t r, int dlead, bool act, uint64_t fi) const {
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q < 6; q++) {
            d[4 * q] = c.x[q].x;
            d[4 * q + 1] = c.x[q].y;
            d[4 * q + 2] = c.x[q].z;
            d[4 * q + 3] = c.x[q].w;
        }
        d[kChunkWords] = c.x6;
        if (EDGE && __any(dlead)) shift_up(d, dlead);
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t ts0 = stamp();
        __builtin_amdgcn_sched_barrier(0);
#endif
        uint32_t w[kChunkWords];
#pragma unroll
#ifdef FCS_ABL_NOALIGN   // measurement-only build: no realignment (wrong CRCs unless r == 0)
        for (int i = 0; i < kChunkWords; i++) w[i] = d[i];
#else
        for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], r);
#endif
#pragma unroll
        for (int i = 0; i < kSingleMaskWords; i++)
            if (4 * i < (int)zmax) w[i] &= m[i];
#ifdef FCS_SINGLE_ONE_CHAIN   // one 24-word chain: no A_48 merge (8 fewer LDS reads per item)
        uint32_t xa = x0 ^ w[0];
#pragma unroll
        for (int i = 0; i < 24; i++) xa = step4(lds, xa, i < 23 ? w[i + 1] : 0u, base0, base1);
        uint32_t v = lane_shift(lds, xa, lanebase);
#else
        uint32_t xa = x0 ^ w[0], xb = w[12];
#pragma unroll
        for (int i = 0; i < 12; i++) {
            xa = step4(lds, xa, i < 11 ? w[i + 1] : 0u, base0, base1);
            xb = step4(lds, xb, i < 11 ? w[13 + i] : 0u, base0, base1);
        }
#ifdef FCS_STAMPS
        asm volatile("" ::"v"(xa), "v"(xb));
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t ts1 = stamp();
        __builtin_amdgcn_sched_barrier(0);
#endif
        uint32_t v = lane_shift(lds, uniform_shift<kLdsH48>(lds, xa, xb), lanebase);
#endif
        v = row_xor(v);
        emit(*kp, lds, act && j == 15, fi, ~v);
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t ts2 = stamp();
        if (dbg != nullptr && (threadIdx.x & 63) == 0) {
            const uint32_t wv = blockIdx.x * (kFixedWgThreads / 64) + (threadIdx.x >> 6);
            atomicAdd((unsigned long long *)&dbg[wv * 4 + 0], (unsigned long long)(ts1 - ts0));
            atomicAdd((unsigned long long *)&dbg[wv * 4 + 1], (unsigned long long)(ts2 - ts0));
            atomicAdd((unsigned long long *)&dbg[wv * 4 + 2], 1ull);
            atomicAdd((unsigned long long *)&dbg[wv * 4 + 3], (unsigned long long)ts2);
        }
#endif
    }
};

__device__ __forceinline__ void issue_raw(uint64_t a, uint32_t r, Raw &c) {
    LoadPriority lp;
#pragma unroll
    for (int q = 0; q < 6; q++) c.x[q] = gload<u32x4a4>(a + 16 * q);
    c.x6 = gload<uint32_t>(a + (r ? 96 : 92));   // 25th dword only matters when r != 0
}

__global__ __launch_bounds__(kFixedWgThreads, 1) void fcs_single_kernel(KParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    stage_tables<kFixedWgThreads>(p, lds);
    init_bad(lds);

    const int lane = threadIdx.x & 63;
    const int j = lane & (kGroup - 1);
    const uint32_t r4 = (uint32_t)(lane & 31) * 4u;
    SingleLane S;
    S.dbg = p.dbg;
    S.kp = &p;
    S.lds = lds;
    S.j = j;
    table_bases(lane, S.base0, S.base1);
    S.lanebase = kLdsLane | r4;
    S.zmax = p.zmax;
    const uint32_t loff = (uint32_t)kChunkBytes * (uint32_t)(j + 1);   // chunk start = end - loff
    {
        int zr = (int)loff - (int)p.flen;
        zr = zr < -1 ? -1 : (zr > kChunkBytes ? kChunkBytes : zr);
#pragma unroll
        for (int i = 0; i < kSingleMaskWords; i++) {
            int t = zr - 4 * i;
            t = t < 0 ? 0 : (t > 4 ? 4 : t);
            S.m[i] = (uint32_t)(0xFFFFFFFFull << (8 * t));
        }
        const uint32_t iv = lds_rd(lds, kLdsInv + 4u * (uint32_t)(zr < 0 ? 0 : (zr > kChunkBytes - 1 ? kChunkBytes - 1 : zr)));
        S.x0 = (zr >= 0 && zr < kChunkBytes) ? iv : 0u;
    }

#ifdef FCS_BLOCKED   // measurement-only build: each workgroup walks its own contiguous frame range
    const uint64_t Q = (uint64_t)kSlotsPerWg<kFixedWgThreads>;
    const uint64_t per = ((p.n + Q - 1) / Q + gridDim.x - 1) / gridDim.x;   // items per workgroup
    const uint64_t f0 = (uint64_t)blockIdx.x * per * Q + threadIdx.x / kGroup;
    const uint64_t lim = (uint64_t)(blockIdx.x + 1) * per * Q < p.n ? (uint64_t)(blockIdx.x + 1) * per * Q : p.n;
    int rem = f0 < lim ? (int)((lim - 1 - f0) / Q) + 1 : 0;
#else
#ifdef FCS_XCD   // measurement-only build: neighbouring frame slots on one XCD (round-robin dispatch)
    const uint32_t wg = (gridDim.x & 7) ? blockIdx.x : (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
#else
    const uint32_t wg = blockIdx.x;
#endif
    const uint64_t Q = (uint64_t)gridDim.x * kSlotsPerWg<kFixedWgThreads>;
    const uint64_t f0 = (uint64_t)wg * kSlotsPerWg<kFixedWgThreads> + threadIdx.x / kGroup;
    int rem = f0 < p.n ? (int)((p.n - 1 - f0) / Q) + 1 : 0;   // items left for this frame slot
#endif
    uint64_t end = p.base + f0 * p.stride + p.flen;
    const uint64_t dend = Q * p.stride;
    uint64_t fi = f0;   // frame index of the item being processed

    // ---- first item: the only one that can start before the arena (frame 0's front lane) ----
    Raw A, B;
    int dlead = 0;
    uint32_t rA = (uint32_t)end & 3u;
    {
        const uint64_t a = rem > 0 ? ((end - loff) & ~3ull) : p.lo4;
        uint64_t ab = a;
        if (__any(a < p.lo4)) {
            dlead = a < p.lo4 ? (int)((p.lo4 - a) >> 2) : 0;
            ab = a < p.lo4 ? p.lo4 : a;
        }
        LoadPriority lp;
#pragma unroll
        for (int q = 0; q < 6; q++) A.x[q] = gload<u32x4a4>(ab + 16 * q);
        A.x6 = gload<uint32_t>(ab + ((rA || dlead) ? 96 : 92));
    }
    uint64_t endB = end + dend;
    uint32_t rB = (uint32_t)endB & 3u;
    issue_raw(rem > 1 ? ((endB - loff) & ~3ull) : p.lo4, rB, B);
    S.process<true>(A, rA, dlead, rem > 0, fi);
    rem -= 1;
    end = endB;
    fi += Q;

    // ---- steady state: two items in flight per lane ----
    while (__any(rem > 0)) {
        const uint64_t endA = end + dend;
        rA = (uint32_t)endA & 3u;
        issue_raw(rem > 1 ? ((endA - loff) & ~3ull) : p.lo4, rA, A);
        S.process<false>(B, rB, 0, rem > 0, fi);
        rem -= 1;
        end = endA;
        fi += Q;
        if (!__any(rem > 0)) break;
        endB = end + dend;
        rB = (uint32_t)endB & 3u;
        issue_raw(rem > 1 ? ((endB - loff) & ~3ull) : p.lo4, rB, B);
        S.process<false>(A, rA, 0, rem > 0, fi);
        rem -= 1;
        end = endB;
        fi += Q;
    }
    flush_bad(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Fixed length, one segment, frames staged through LDS by DMA (fcs_dma_kernel; host-selected for
// kDmaMinLen..kDmaCover bytes, e.g. the 1518-B benchmark frames, when four consecutive frames fit
// a 6 KiB slot: fixed_dma()).
// A wave's item is four consecutive frames, as in fcs_single_kernel. The wave copies the item's
// bytes into one of its LDS slots with six global_load_lds_dwordx4 (each 1 KiB contiguous:
// coalesced rows, no VGPR destination, non-temporal since every line is read exactly once), then
// lane c of each frame reads its 96-byte window [E - e_c - 96, E - e_c) from the slot (25 dwords,
// realigned with v_alignbyte; the window offsets e_c = dma_end_off(c) put one frame's 16 windows on
// 16 distinct banks) and runs two slice-by-4 chains, the A_48 merge, the lane shift A_{e_c} and the
// row XOR. One slot per wave, 16 waves per CU: the DMA of a wave's next item is issued as soon as
// the current item's words are in registers, so it lands while the CRC work runs.
// Items: a static interleaved share (item wid + k W for wave wid of W) and, for large batches
// (p.ctr != null), a dynamic tail: the remaining items are handed out in chunks by a device
// counter, chunk sizes shrinking with the work left (guided), the next chunk requested one chunk
// ahead. Without it the waves' finishing times spread over 18 % of the kernel (slower XCDs and
// CUs), and the kernel ends with the slowest (tools/stamps_dma.py).
//
// LDS (160 KiB): a 64 KiB table image of 256 rows of 256 B (row = byte value e) and the slots.
//   row bytes [0, 128): slice tables, slot s = T_{3-s}[e] x 8 replicas (lookups: step4_l8);
//   row bytes [128, 256) ("hole" e): hole 16 t + n = nibble n of the lane tables' table t for the
//     32 lane slots; holes 128.. the chain-merge tables, then INV, then the verify counters.
// ---------------------------------------------------------------------------------------------
// (constants, table staging, slice step, shifts and the slot DMA: fcs_crc.hpp)
// MW: words a front mask can touch (host-selected: 2 when the front lane masks at most 8 bytes,
// i.e. len >= 1516, else kSingleMaskWords).
// STREAM: the measurement form behind fcs_dma_stream_dev: the same slot DMA, schedule and window
// reads, no CRC work (bench.py's LDS-DMA read ceiling beside the plain read stream).
template <int MW, bool STREAM>
__global__ __launch_bounds__(kDmaWgThreads, 1) void fcs_dma_kernel(KParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDmaLdsBytes];
    const int tid = threadIdx.x;
    stage_dma_tables(p, lds, tid);
    init_bad<kDmaBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const int c = lane & (kGroup - 1);     // chunk index back from the frame end
    const int g = lane >> 4;               // frame of the item
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *slot0 = lds + kDmaRing + (uint32_t)wave * kDmaItemBytes;
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    const uint32_t lanebase = kDmaHole + (uint32_t)(lane & 31) * 4u;

    // loop invariants: window offset within the item, front masks, INV start of the front lane
    const uint32_t ec = dma_end_off(c);
    const int64_t klane = (int64_t)g * (int64_t)p.stride + (int64_t)p.flen - (int64_t)ec - kChunkBytes;
    const int zc = (c == kGroup - 1) ? (int)(kDmaCover - p.flen) : (dma_short_lane(c) ? 4 : 0);
    static_assert(MW >= 1 && MW <= kSingleMaskWords, "mask words");
    uint32_t m[MW];
#pragma unroll
    for (int i = 0; i < MW; i++) {
        int t = zc - 4 * i;
        t = t < 0 ? 0 : (t > 4 ? 4 : t);
        m[i] = (uint32_t)(0xFFFFFFFFull << (8 * t));
    }
    const uint32_t x0 = (c == kGroup - 1) ? lds_rd(lds, dma_hole(kDmaInvHole + (uint32_t)zc / 32u) + (uint32_t)(zc % 32) * 4u)
                                          : 0u;

    // Slots are whole 16-B pieces: reads stay inside [floor16(lo4), ceil16(hi4)), i.e. up to 12 bytes
    // before the arena's first and after its last dword (never across a page: pages are 4 KiB
    // aligned). Those bytes land in the slot but lie outside every window's frame bytes.
    const uint64_t lo16 = p.lo4 & ~15ull;
    const uint64_t smax = ((p.hi4 + 15) & ~15ull) - kDmaItemBytes;   // last slot start inside the arena
    auto slot_src = [&](uint64_t S) {
        const uint64_t a = S & ~15ull;
        return a < lo16 ? lo16 : (a > smax ? smax : a);
    };
    // ---- items (4 frames each), from the dispenser ----
    constexpr uint64_t kEnd = Dispenser::kEnd;
    Dispenser D(p.ctr, (p.n + 3) >> 2, (uint64_t)gridDim.x * kDmaWaves,
                (uint64_t)blockIdx.x * kDmaWaves + (uint64_t)wave, lane, FCS_DMA_DYN_PCT, 4, FCS_DMA_CHUNK_MAX);
    D.align = 16;   // chunks start on 16-item groups: whole 256-B result runs
    auto item_start = [&](uint64_t i) { return p.base + 4 * i * p.stride; };   // first frame of item i
    // slot bytes an item's windows read: up to its last frame's end plus the realignment dword
    auto item_need = [&](uint64_t S, uint64_t src) {
        const uint64_t e = S + 3 * p.stride + p.flen + 4 - src;
        return (uint32_t)(e < (uint64_t)kDmaItemBytes ? e : (uint64_t)kDmaItemBytes);
    };
    auto dma_of = [&](const uint8_t *slot, uint64_t i) {
#ifdef FCS_DMA_PRIO   // measurement-only: the slot DMA issued at raised wave priority
        LoadPriority lp;
#endif
        const uint64_t S = item_start(i), sn = slot_src(S);
        dma_item(slot, sn, lane, item_need(S, sn));
    };

    uint64_t it = D.first();
    if (it != kEnd) dma_of(slot0, it);
    uint32_t cbuf = 0;    // FCSs of the current run of items, lane 4 (item & 15) + frame
    uint64_t cmask = 0;   // lanes of cbuf that hold one (wave-uniform)

#ifdef FCS_STAMPS   // measurement-only: per-wave cycles waiting for the slot vs. the whole item
    uint64_t st_wait = 0, st_all = 0, st_items = 0;
    const uint64_t st_rt0 = __builtin_amdgcn_s_memrealtime(), st_c0 = __builtin_amdgcn_s_memtime();
#endif
    while (it != kEnd) {   // wave-uniform
        const uint8_t *slot = slot0;
        const uint64_t f = 4 * it;
        const uint64_t S = item_start(it);
        const uint64_t src = slot_src(S);
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t ts0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
#endif
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's slot DMA has landed
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t ts1 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
        st_wait += ts1 - ts0;
#endif
        const int64_t x = (int64_t)(S - src) + klane;   // window start within the slot (>= -28)
        const uint32_t r = (uint32_t)x & 3u;
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(slot + (x & ~3ll));
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q < kChunkWords; q++) d[q] = wp[q];
        {   // the 25th dword matters only when r != 0; then it lies inside the slot. Clamped so the
            // last slot in LDS is never read past its end.
            const uint64_t a24 = (uint64_t)(wp + kChunkWords), lim = (uint64_t)(slot + kDmaItemBytes - 4);
            d[kChunkWords] = *reinterpret_cast<const uint32_t *>(a24 < lim ? a24 : lim);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA
        const uint64_t nxt = D.next(it);
        if (nxt != kEnd) dma_of(slot, nxt);

        if (STREAM) {   // read ceiling: the words are only XORed together
            uint32_t acc = r;
#pragma unroll
            for (int q = 0; q <= kChunkWords; q++) acc ^= d[q];
            if (acc == 0x9E3779B9u) p.out[0] = acc;   // keeps the reads live; practically never stores
            it = nxt;
#ifdef FCS_STAMPS
            st_all += __builtin_amdgcn_s_memtime() - ts0;
            st_items++;
#endif
            continue;
        }
        uint32_t w[kChunkWords];
#pragma unroll
#ifdef FCS_DMA_ABL_NOALIGN   // measurement-only: no realignment (wrong FCS unless r == 0)
        for (int i = 0; i < kChunkWords; i++) w[i] = d[i] ^ (i == 0 ? r : 0u);
#else
        for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], r);
#endif
#pragma unroll
        for (int i = 0; i < MW; i++) w[i] &= m[i];
        // kDmaChains independent chains of CL words; chain h ends 4 CL (kDmaChains - 1 - h) bytes
        // before the window end, so the window value is XOR_h A_{4 CL (kDmaChains - 1 - h)}(chain h)
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
        uint32_t v = lane_shift_dma(lds, mv, lanebase);
        v = row_xor(v);
        // Results of a run of consecutive items collect in one register (lane 4 k + g: frame g of
        // item k of a 16-item group) and leave as one coalesced store of up to 256 B: a 16-B store
        // per item, whose 128-B line the L2 evicted half-written before the next items filled it,
        // cost 2x the CRC bytes in HBM writes (WRITE_SIZE).
        {
            const uint32_t k = (uint32_t)(it & 15u);
            const uint32_t vq = (uint32_t)__shfl((int)~v, (lane & 3) * kGroup);   // frame (lane & 3)'s FCS
            if ((uint32_t)(lane >> 2) == k) cbuf = vq;
            const uint64_t live = f + 4 <= p.n ? 0xFull : ((1ull << (p.n - f)) - 1ull);
            cmask |= live << (4 * k);
            if (k == 15 || nxt != it + 1) {
                emit<kDmaBad>(p, lds, (cmask >> lane) & 1ull, 4 * (it & ~15ull) + (uint64_t)lane, cbuf);
                cmask = 0;
            }
        }
        it = nxt;
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        st_all += __builtin_amdgcn_s_memtime() - ts0;
        st_items++;
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
#ifdef FCS_STAMPS
    if (p.dbg != nullptr && lane == 0) {
        const uint32_t wv = blockIdx.x * kDmaWaves + (uint32_t)wave;
        p.dbg[wv * 8 + 0] = st_wait;
        p.dbg[wv * 8 + 1] = st_all;
        p.dbg[wv * 8 + 2] = st_items;
        const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
        p.dbg[wv * 8 + 3] = rt1 - st_rt0;
        p.dbg[wv * 8 + 4] = __builtin_amdgcn_s_memtime() - st_c0;
        p.dbg[wv * 8 + 5] = st_rt0;
        p.dbg[wv * 8 + 6] = rt1;
        p.dbg[wv * 8 + 7] = __builtin_amdgcn_s_getreg(/*HW_REG_XCC_ID*/ (20 << 0) | (0 << 6) | (3 << 11));
    }
#endif
    flush_bad<kDmaBad>(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Fixed length just over the LDS-DMA kernel's cover (fcs_wide_kernel<WD>; host-selected by
// wide_wd(): kWideMinLen..kWideCover bytes, four consecutive frames per slot).
// fcs_dma_kernel with wider lane windows of WD dwords (WD = 32: 128 B, 8 KiB slots, 12 waves, up to
// 1988 B; WD = 26: 104 B, 7 KiB slots, 13 waves, up to 1604 B). Lane c of a frame's 16 reads
// [E - s c - 4 WD, E - s c) with s = 4 WD - 4 (E = frame end), WD + 1 dwords from the slot,
// realigned. A window's first word is the next lane's last, so every live lane masks it, except the
// front lane cf = (len - 1) / s (the last whose window reaches into the frame), which masks its
// zc = s cf + 4 WD - len leading bytes and starts its chain from INV[zc]; lanes past cf are dropped.
// cf and zc are launch constants (the length is fixed), so the masks are scalars. Two chains
// (16 + 16 or 12 + 14 words) merged with A_{4 (WD - CL0)}, lane shift A_{s c}, row XOR, the LDS-DMA
// kernel's 256-B result runs. The generic register-load kernel spends two 1536-B segments on a
// 1600-B frame; this one covers it in one item.
// LDS: the 64 KiB table image (slice tables; holes 0..127 the lane tables A_{s c}, 128..131 the
// merge, 132..135 INV[0..127], then the verify counters) and the slots.
// CPU model: tests/kernel_model.py model_wide_item.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kWideMergeHole = 128, kWideInvHole = 132;
constexpr uint32_t kWideBad = dma_hole(kWideInvHole + 4);
__host__ __device__ constexpr uint32_t wide_lds_bytes(int wd) {
    return kDmaRing + (uint32_t)(wide_threads(wd) / 64) * wide_slot(wd);
}
static_assert(wide_lds_bytes(32) <= 163840 && wide_lds_bytes(26) <= 163840 && wide_lds_bytes(kWideMidMax) <= 163840,
              "LDS per CU");
static_assert(kDmaMergeHole == kWideMergeHole, "merge_shift_dma reads merge table 0 at the same holes");
// chain split: chain 0 = words [0, CL0), chain 1 = [CL0, WD); chain 1 spans 4 (WD - CL0) bytes, a
// multiple of 8 so that its merge A_{4 (WD - CL0)} is one of the blob's A_{8 k} (k <= 11)
__host__ __device__ constexpr int wide_cl0(int wd) {
    return wd == 32 ? 16 : (wd == 30 ? 14 : (wd == 26 ? 12 : wd - 2 * (wd / 4)));
}

template <int WD, int G, int NT = wide_threads(WD)>   // NT: the workgroup size (the staging stride)
__device__ __forceinline__ void stage_wide_tables(const KParams &p, uint8_t *lds, int tid) {
    static_assert(G == 16 ? (WD == 26 || WD == 30 || WD == 32 || wide_mid_ok(WD))
                          : (G == 8 ? wide8_ok(WD) : (G == 4 && wide4_ok(WD))), "window width");
    constexpr uint32_t kLane = G == 4 ? kBlobLane4 + (uint32_t)(WD - kWide4Min) * 4096u
                             : G == 8 ? kBlobLane8 + (uint32_t)(WD - kWide8Min) * 4096u
                             : WD == 32 ? kBlobLaneWide
                                        : (WD == 30 ? kBlobLaneWide30
                                                    : (WD == 26 ? kBlobLaneWide26 : kBlobLaneMid + (uint32_t)(WD - kWideMidMin) * 4096u));
    constexpr int kMergeK = 2 * (WD - wide_cl0(WD)) / 4;   // A_{8 k} with 8 k = 4 (WD - CL0)
    static_assert((WD - wide_cl0(WD)) % 2 == 0 && kMergeK >= 1 && kMergeK <= 11, "merge table");
    for (int i = tid; i < 2048; i += NT) {   // slice tables as fcs_dma_kernel
        const uint32_t v = p.blob[kBlobSlice + 256 * (3 - ((i & 7) >> 1)) + (i >> 3)];
        u32x4 vv = {v, v, v, v};
        *reinterpret_cast<u32x4 *>(lds + (uint32_t)(i >> 3) * 256u + (uint32_t)(i & 7) * 16u) = vv;
    }
    for (int i = tid; i < 4096; i += NT)   // lane tables [t][n][slot]: hole 16 t + n
        *reinterpret_cast<uint32_t *>(lds + dma_hole((uint32_t)i >> 5) + (uint32_t)(i & 31) * 4u) = p.blob[kLane + i];
    for (int i = tid; i < 128; i += NT) {   // the chain merge
        const int t = (i >> 4) & 7, e = i & 15;
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kWideMergeHole + (uint32_t)(t >> 1)) + 64u * (uint32_t)(t & 1) +
                                      4u * (uint32_t)e) = p.blob[kBlobMerge + (kMergeK - 1) * 128 + i];
    }
    for (int i = tid; i < (int)kWideWin; i += NT)
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kWideInvHole + (uint32_t)i / 32u) + (uint32_t)(i % 32) * 4u) =
            p.blob[kBlobInvWide + i];
}

// The slot DMA: six, seven or eight 1 KiB rows from two address registers, each only as far as the
// item's bytes reach; the first and last rows at the default cache policy, the middle ones
// non-temporal.
template <int WD>
__device__ __forceinline__ void wide_dma_item(const uint8_t *slot, uint64_t src, int lane, uint32_t need) {
    typedef __attribute__((address_space(3))) void lds_void;
    const uint64_t a = src + 16 * (uint64_t)lane, b = a + 4096;
    lds_void *la = (lds_void *)slot, *lb = (lds_void *)(slot + 4096);
    const uint32_t o = 16u * (uint32_t)lane;
    __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 0, FCS_DMA_EDGE_AUX);
    if (1024u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 1024, FCS_DMA_AUX);
    if (2048u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 2048, FCS_DMA_AUX);
    if (3072u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), la, 16, 3072, FCS_DMA_AUX);
    if (4096u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 0, FCS_DMA_AUX);
    if constexpr (wide_slot(WD) == 6 * 1024) {   // six rows: the last one at the edge policy
        if (5120u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 1024, FCS_DMA_EDGE_AUX);
    } else if constexpr (WD == 32) {
        if (5120u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 1024, FCS_DMA_AUX);
        if (6144u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 2048, FCS_DMA_AUX);
        if (7168u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 3072, FCS_DMA_EDGE_AUX);
    } else {
        static_assert(wide_slot(WD) == 7 * 1024, "seven rows");
        if (5120u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 1024, FCS_DMA_AUX);
        if (6144u + o < need) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(b), lb, 16, 2048, FCS_DMA_EDGE_AUX);
    }
}

// G: lanes per frame (16: four frames per item; 8: eight frames per item, eight windows each).
template <int WD, int G = 16>
__global__ __launch_bounds__(wide_threads(WD), 1) void fcs_wide_kernel(KParams p) {
    constexpr uint32_t kWin = wide_win(WD), kStep = wide_step(WD), kSlot = wide_slot(WD);
    constexpr uint32_t kLdsB = wide_lds_bytes(WD);
    constexpr int kWaves = wide_threads(WD) / 64, CL0 = wide_cl0(WD);
    static_assert(G == 16 || G == 8 || G == 4, "lanes per frame");
    constexpr int kFr = 64 / G;   // frames per item
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsB];
    const int tid = threadIdx.x;
    stage_wide_tables<WD, G>(p, lds, tid);
    init_bad<kWideBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const int c = lane & (G - 1);          // window index back from the frame end
    const int g = lane / G;                // frame of the item
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *slot = lds + kDmaRing + (uint32_t)wave * kSlot;
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    const uint32_t lanebase = kDmaHole + (uint32_t)(lane & 31) * 4u;

    // launch constants: the front lane, its leading bytes, the words they reach (scalars)
    const int cf = (int)((p.flen - 1u) / kStep) < G - 1 ? (int)((p.flen - 1u) / kStep) : G - 1;
    const uint32_t zc = kStep * (uint32_t)cf + kWin - p.flen;   // 0 .. kWin - 1
    const uint32_t mwords = (zc + 3u) / 4u;
    const bool live = c <= cf, front = c == cf;
    const uint32_t x0 = front ? lds_rd(lds, dma_hole(kWideInvHole + zc / 32u) + (zc % 32u) * 4u) : 0u;
    const uint32_t m0 = front ? (zc >= 4u ? 0u : (uint32_t)(0xFFFFFFFFull << (8u * zc))) : 0u;
    uint32_t keep = front ? 0u : 0xFFFFFFFFu;
    asm volatile("" : "+v"(keep));   // opaque: kept a register, not re-derived as a per-word select
    const int64_t klane = (int64_t)g * (int64_t)p.stride + (int64_t)p.flen - (int64_t)(kStep * (uint32_t)c) - (int64_t)kWin;

    // slots are whole 16-B pieces inside [floor16(lo4), ceil16(hi4)) (as fcs_dma_kernel's)
    const uint64_t lo16 = p.lo4 & ~15ull;
    const uint64_t smax = ((p.hi4 + 15) & ~15ull) - kSlot;
    auto slot_src = [&](uint64_t S) {
        const uint64_t a = S & ~15ull;
        return a < lo16 ? lo16 : (a > smax ? smax : a);
    };
    auto item_start = [&](uint64_t i) { return p.base + (uint64_t)kFr * i * p.stride; };
    auto dma_of = [&](uint64_t i) {
        const uint64_t S = item_start(i), src = slot_src(S);
        const uint64_t e = S + (uint64_t)(kFr - 1) * p.stride + p.flen + 4 - src;
        wide_dma_item<WD>(slot, src, lane, (uint32_t)(e < (uint64_t)kSlot ? e : (uint64_t)kSlot));
    };

    constexpr uint64_t kEnd = Dispenser::kEnd;
    Dispenser D(p.ctr, (p.n + kFr - 1) / kFr, (uint64_t)gridDim.x * kWaves,
                (uint64_t)blockIdx.x * kWaves + (uint64_t)wave, lane, FCS_DMA_DYN_PCT, 4, FCS_DMA_CHUNK_MAX);
    D.align = G;   // chunks start on G-item groups: whole 256-B result runs
    uint64_t it = D.first();
    if (it != kEnd) dma_of(it);
    uint32_t cbuf = 0;    // FCSs of the current run of items, lane kFr (item mod G) + frame
    uint64_t cmask = 0;   // lanes of cbuf that hold one (wave-uniform)
    while (it != kEnd) {   // wave-uniform
        const uint64_t f = (uint64_t)kFr * it;
        const uint64_t S = item_start(it);
        const uint64_t src = slot_src(S);
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's slot DMA has landed
        // window start within the slot: >= -128 for live lanes (the front lane's masked bytes may lie
        // before the slot; they are read from the LDS below it and masked). Lanes past the front lane
        // read wherever their window falls (clamped to the LDS allocation) and are dropped.
        int64_t x = (int64_t)(S - src) + klane;
        x = x < -(int64_t)kDmaRing ? -(int64_t)kDmaRing : x;
        const uint32_t r = (uint32_t)x & 3u;
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(slot + (x & ~3ll));
        uint32_t d[WD + 1];
#pragma unroll
        for (int q = 0; q < WD; q++) d[q] = wp[q];
        {   // the last dword matters only when r != 0; clamped so the last slot is never read past its end
            const uint64_t al = (uint64_t)(wp + WD), lim = (uint64_t)(lds + kLdsB - 4);
            d[WD] = *reinterpret_cast<const uint32_t *>(al < lim ? al : lim);
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA
        const uint64_t nxt = D.next(it);
        if (nxt != kEnd) dma_of(nxt);

        uint32_t w[WD];
#pragma unroll
        for (int i = 0; i < WD; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], r);
        // masks: word 0 of every live lane (its neighbour's last word) except the front lane's, whose
        // first zc bytes go (scalar masks, words below the launch-uniform bound only)
#ifdef FCS_WIDE_OLD_MASK   // measurement-only: round-3 form (a select and an AND per word)
        w[0] &= front ? (zc >= 4u ? 0u : (uint32_t)(0xFFFFFFFFull << (8u * zc))) : 0u;
#pragma unroll
        for (int i = 1; i < WD; i++) {
            if ((uint32_t)i < mwords) {
                const int t = (int)zc - 4 * i;
                const uint32_t mk = t >= 4 ? 0u : (uint32_t)(0xFFFFFFFFull << (8 * (t < 0 ? 0 : t)));
                w[i] &= front ? mk : 0xFFFFFFFFu;
            }
        }
#else
        // word 0 by a per-lane loop invariant; word i >= 1 by mk_i | keep (keep = ~0 outside the front
        // lane), which the compiler hoists into a register per word: one AND per word and item. (A
        // branch on the launch-uniform mwords was if-converted into a select per word.)
        (void)mwords;
        w[0] &= m0;
#pragma unroll
        for (int i = 1; i < WD; i++) {
            const int t = (int)zc - 4 * i;
            const uint32_t mk = t >= 4 ? 0u : (uint32_t)(0xFFFFFFFFull << (8 * (t < 0 ? 0 : t)));
            w[i] &= mk | keep;
        }
#endif
        // chain 0 over words [0, CL0), chain 1 over [CL0, WD), run side by side
        uint32_t xa = w[0] ^ x0, xb = w[CL0];
        constexpr int CL1 = WD - CL0, CLM = CL0 > CL1 ? CL0 : CL1;   // either chain may be the longer one
#pragma unroll
        for (int i = 0; i < CLM; i++) {
            if (i < CL0) xa = step4_l8(lds, xa, i < CL0 - 1 ? w[i + 1] : 0u, B, SEL);
            if (i < CL1) xb = step4_l8(lds, xb, i < CL1 - 1 ? w[CL0 + i + 1] : 0u, B, SEL);
        }
        const uint32_t mv = merge_shift_dma(lds, 0, xa, xb);
        uint32_t v = live ? lane_shift_dma(lds, mv, lanebase) : 0u;
        if constexpr (G == 16) {
            v = row_xor(v);
        } else {   // the eight-lane half-row (or four-lane quad) sums: row_xor's first steps
            v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad [1,0,3,2]
            v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad [2,3,0,1]
            if constexpr (G == 8)
                v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
        }
        {
            const uint32_t k = (uint32_t)(it & (uint64_t)(G - 1));
            const uint32_t vq = (uint32_t)__shfl((int)~v, (lane % kFr) * G);   // frame (lane mod kFr)'s FCS
            if ((uint32_t)(lane / kFr) == k) cbuf = vq;
            constexpr uint64_t kAll = (1ull << kFr) - 1ull;
            const uint64_t livem = f + kFr <= p.n ? kAll : ((1ull << (p.n - f)) - 1ull);
            cmask |= livem << (kFr * k);
            if (k == (uint32_t)(G - 1) || nxt != it + 1) {
                emit<kWideBad>(p, lds, (cmask >> lane) & 1ull, (uint64_t)kFr * (it & ~(uint64_t)(G - 1)) + (uint64_t)lane, cbuf);
                cmask = 0;
            }
        }
        it = nxt;
    }
    flush_bad<kWideBad>(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Fixed length over 1524 B, any stride: frame-interleaved segments staged through LDS by DMA
// (fcs_segil_kernel; host-selected by fixed_segil()).
// A frame of L bytes is cut from its front into m = ceil(L / 1524) segments: a front segment of
// Lf = L - 1524 (m - 1) bytes, then m - 1 segments of exactly 1524 bytes. A wave's unit is four
// frames, one per quarter-wave; item r of a unit is segment r of its four frames: four runs of at
// most 97 16-B pieces (the segment plus the alignment of its ends), each DMAed into its own 2 KiB
// part of the wave's 8 KiB slot (two rows: 64 + 33 lanes). A 1524-B segment is exactly the cover
// of fcs_dma_kernel's 16 lane windows, so it needs no mask beyond the short lanes' overlap word,
// and the frame's CRC state after the previous segment enters through lane 15's chain start (a CRC
// state is the same as XORing it into the next four data bytes). No shift is needed between
// segments: the quarter's row XOR after segment r is its frame's CRC state after that segment,
// and stays in a register until the next item. The front item (1 in m) masks each lane's bytes
// before the frame start (loop-invariant per lane: Lf is fixed), drops lanes wholly before it and
// injects INV at the frame's first byte.
// LDS: the 64 KiB table image of fcs_dma_kernel, then 12 slots of 8 KiB (160 KiB).
// ---------------------------------------------------------------------------------------------
constexpr int kSegilWaves = 12;
constexpr int kSegilThreads = kSegilWgThreads;
static_assert(kSegilThreads == 64 * kSegilWaves, "12 waves");
constexpr uint32_t kSegilRunBytes = 2048;                      // one run's part of a slot
constexpr uint32_t kSegilSlotBytes = 4 * kSegilRunBytes;
constexpr uint32_t kSegilLdsBytes = kDmaRing + (uint32_t)kSegilWaves * kSegilSlotBytes;
static_assert(kSegilLdsBytes <= 163840, "LDS per CU");
static_assert(kSegilWaves <= 16, "verify counters: 16 waves");
#ifndef FCS_SEGIL_TAIL_AUX   // cache policy of a run's second row (it holds the line the next segment shares)
#define FCS_SEGIL_TAIL_AUX 0
#endif
#ifndef FCS_SEGIL_SKEW   // bytes added to odd runs' LDS base (bank phase of their windows)
#define FCS_SEGIL_SKEW 16
#endif

// One run's DMA: pieces 0..63 in row 0 (non-temporal), 64..need-1 in row 1.
__device__ __forceinline__ void segil_run(const uint8_t *dst, uint64_t src, int lane, uint32_t pieces) {
    typedef __attribute__((address_space(3))) void lds_void;
    const uint64_t a = src + 16 * (uint64_t)lane;
    lds_void *l = (lds_void *)dst;
    if ((uint32_t)lane < pieces) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), l, 16, 0, FCS_DMA_AUX);
    if ((uint32_t)lane + 64u < pieces)
        __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), l, 16, 1024, FCS_SEGIL_TAIL_AUX);
}

__global__ __launch_bounds__(kSegilThreads, 1) void fcs_segil_kernel(KParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSegilLdsBytes];
    const int tid = threadIdx.x;
    stage_dma_tables<kSegilThreads>(p, lds, tid);
    init_bad<kDmaBad>(lds);
    __syncthreads();

    // ---- frame geometry (wave-uniform) ----
    const uint32_t L = p.flen;
    const uint32_t m = (L + kDmaCover - 1) / kDmaCover;   // segments, >= 2
    const uint32_t Lf = L - kDmaCover * (m - 1);          // front segment, 1 .. 1524

    const int lane = tid & 63;
    const int c = lane & (kGroup - 1);        // window index back from the segment end
    const uint32_t q = (uint32_t)lane >> 4;   // quarter: frame 4 u + q of unit u
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *slot = lds + kDmaRing + (uint32_t)wave * kSegilSlotBytes;
    const uint8_t *run = slot + q * kSegilRunBytes + (q & 1u) * FCS_SEGIL_SKEW;
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    const uint32_t lanebase = kDmaHole + (uint32_t)(lane & 31) * 4u;
    const uint32_t ec = dma_end_off(c);

    // loop invariants. Other segments: the short lanes' overlap word. Front segment: zr bytes of
    // the lane's window lie before the frame start (>= 96: the whole window, the lane is dropped);
    // the lane holding the first byte in its unmasked part starts its chain from INV there.
    const uint32_t mn0 = dma_short_lane(c) ? 0u : 0xFFFFFFFFu;
    const int zr = (int)(kDmaCover - Lf) - (int)(kDmaCover - ec - kChunkBytes);
    const bool fdead = zr >= kChunkBytes;
    int zf = zr < 0 ? 0 : (zr > kChunkBytes ? kChunkBytes : zr);
    if (dma_short_lane(c) && zf < 4) zf = 4;
    const uint32_t x0f = (!fdead && zr >= 0 && zf == zr)
                             ? lds_rd(lds, dma_hole(kDmaInvHole + (uint32_t)zr / 32u) + (uint32_t)(zr % 32) * 4u)
                             : 0u;
    const int zb = fdead ? 0 : zf;   // the wave masks word groups up to its largest live claim
    // front word groups any live lane needs masked: one scalar (as six hoisted lane masks they took
    // SGPRs the kernel then spilled)
    uint32_t gmask = 0;
#pragma unroll
    for (int g = 0; g < kChunkWords / 4; g++)
        if (__any(zb > 16 * g)) gmask = (uint32_t)g + 1u;
    gmask = (uint32_t)__builtin_amdgcn_readfirstlane((int)gmask);

    const uint64_t n = p.n, units = (n + 3) >> 2;
    // chunks of about 64 items, and at least 16 units so that result runs fill 256-B groups; jumbo
    // frames (m >= 4) up to 32 units: each chunk is one device-scope atomic on the work counter, and
    // at 16 units those were 13 % on top of the CRC bytes in WRITE_SIZE. Frames of
    // m > 6 items take at most about kSegilChunkItems items per chunk, so that the last chunks still
    // balance across the waves (tools/ab.py, round 4: 16384 B +3 %, 65536 B +10.6 %; 9000 B, m = 6,
    // unchanged).
#ifndef FCS_SEGIL_CMAX_ITEMS   // measurement-only override
#define FCS_SEGIL_CMAX_ITEMS 192
#endif
    constexpr uint32_t kSegilChunkItems = FCS_SEGIL_CMAX_ITEMS;
    const uint32_t cmax = m >= 4 ? (kSegilChunkItems / m > 32u ? 32u : (kSegilChunkItems / m < 1u ? 1u : kSegilChunkItems / m))
                                 : 64u / m;
    Dispenser D(p.ctr, units, (uint64_t)gridDim.x * kSegilWaves, (uint64_t)blockIdx.x * kSegilWaves + (uint64_t)wave,
                lane, 100, 1, cmax);
    D.align = 16;
    constexpr uint64_t kEnd = Dispenser::kEnd;
    // segment r of frame f: [start, start + len); the run starts at the 16-B boundary below it
    auto seg_start = [&](uint64_t f, uint32_t r) {
        return p.base + f * p.stride + (r ? (uint64_t)Lf + (uint64_t)kDmaCover * (r - 1) : 0ull);
    };
    auto issue = [&](uint64_t u, uint32_t r) {   // the item's four runs (wave-uniform control)
        const uint32_t len = r ? kDmaCover : Lf;
#pragma unroll
        for (uint32_t qq = 0; qq < 4; qq++) {
            const uint64_t f = 4 * u + qq;
            if (f < n) {
                const uint64_t s0 = seg_start(f, r), a = s0 & ~15ull;
                const uint32_t pieces = (uint32_t)((((s0 + len) + 15) & ~15ull) - a) >> 4;
                segil_run(slot + qq * kSegilRunBytes + (qq & 1u) * FCS_SEGIL_SKEW, a, lane, pieces);
            }
        }
    };

    uint64_t u = D.first();
    uint32_t r = 0;
    if (u != kEnd) issue(u, 0);
    uint32_t acc = 0;   // this quarter's frame: CRC state after its segments so far
    uint32_t cbuf = 0;    // FCSs of the current run of units, lane 4 (unit & 15) + frame
    uint64_t cmask = 0;   // lanes of cbuf that hold one (wave-uniform)
#ifdef FCS_STAMPS   // measurement-only: per-wave slot wait, finishing time, XCD and clock (as fcs_dma_kernel)
    uint64_t st_wait = 0, st_all = 0, st_items = 0;
    const uint64_t st_rt0 = __builtin_amdgcn_s_memrealtime(), st_c0 = __builtin_amdgcn_s_memtime();
#endif
    while (u != kEnd) {   // wave-uniform
        const uint64_t f = 4 * u + q;
        const bool act = f < n;
        const uint64_t s0 = act ? seg_start(f, r) : 0ull;
        const uint32_t len = r ? kDmaCover : Lf;
        const int64_t x = (int64_t)(s0 & 15ull) + (int64_t)len - (int64_t)ec - kChunkBytes;   // window start in the run
        const uint32_t ra = (uint32_t)x & 3u;
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        const uint64_t ts0 = __builtin_amdgcn_s_memtime();
        __builtin_amdgcn_sched_barrier(0);
#endif
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's runs have landed
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        st_wait += __builtin_amdgcn_s_memtime() - ts0;
        __builtin_amdgcn_sched_barrier(0);
#endif
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(run + (x & ~3ll));
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int i = 0; i <= kChunkWords; i++) d[i] = wp[i];
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA

        // ---- the next item: the next segment of the unit, or the dispenser's next unit ----
        uint64_t un = u;
        uint32_t rn = r + 1;
        if (rn == m) {
            un = D.next(u);
            rn = 0;
        }
        if (un != kEnd) issue(un, rn);

        // ---- this item ----
#ifdef FCS_SEGIL_NOCRC   // measurement-only: the window words XORed instead of the CRC work (wrong FCS)
        {
            uint32_t xx = ra;
#pragma unroll
            for (int i = 0; i <= kChunkWords; i++) xx ^= d[i];
            acc = row_xor(xx ^ acc);
        }
        if (false) {
#endif
        uint32_t w[kChunkWords];
#pragma unroll
        for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], ra);
        uint32_t x0;
        if (r == 0) {
            const int zf8 = 8 * zf;
            // an opaque copy: hoisted out of the item loop, the six group tests would each take an
            // SGPR pair (twelve SGPRs, which the kernel then spilled to VGPR lanes)
            uint32_t gm = gmask;
            asm volatile("" : "+s"(gm));
#pragma unroll
            for (int g = 0; g < kChunkWords / 4; g++) {
                if ((uint32_t)g >= gm) break;
#pragma unroll
                for (int i = 4 * g; i < 4 * g + 4; i++) {
                    // zf is a loop invariant: the compiler hoists this clamp (no v_med3 asm here)
                    int t = zf8 - 32 * i;
                    t = t < 0 ? 0 : (t > 32 ? 32 : t);
                    w[i] &= (uint32_t)(0xFFFFFFFFull << t);
                }
            }
            x0 = x0f;
        } else {
            w[0] &= mn0;
            x0 = c == kGroup - 1 ? acc : 0u;
        }
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
        uint32_t v = lane_shift_dma(lds, mv, lanebase);
        if (r == 0 && fdead) v = 0u;
        acc = row_xor(v);
#ifdef FCS_SEGIL_NOCRC
        }
#endif
        if (r == m - 1) {   // results of consecutive units leave as one coalesced store (as fcs_dma_kernel)
            const uint32_t k = (uint32_t)(u & 15u);
            const uint32_t vq = (uint32_t)__shfl((int)~acc, (lane & 3) * kGroup);
            if ((uint32_t)(lane >> 2) == k) cbuf = vq;
            const uint64_t f0 = 4 * u;
            cmask |= (f0 + 4 <= n ? 0xFull : ((1ull << (n - f0)) - 1ull)) << (4 * k);
            if (k == 15 || un != u + 1) {
                emit<kDmaBad>(p, lds, (cmask >> lane) & 1ull, 4 * (u & ~15ull) + (uint64_t)lane, cbuf);
                cmask = 0;
            }
        }
        u = un;
        r = rn;
#ifdef FCS_STAMPS
        __builtin_amdgcn_sched_barrier(0);
        st_all += __builtin_amdgcn_s_memtime() - ts0;
        st_items++;
        __builtin_amdgcn_sched_barrier(0);
#endif
    }
#ifdef FCS_STAMPS
    if (p.dbg != nullptr && lane == 0) {
        const uint32_t wv = blockIdx.x * kSegilWaves + (uint32_t)wave;
        const uint64_t rt1 = __builtin_amdgcn_s_memrealtime();
        p.dbg[wv * 8 + 0] = st_wait;
        p.dbg[wv * 8 + 1] = st_all;
        p.dbg[wv * 8 + 2] = st_items;
        p.dbg[wv * 8 + 3] = rt1 - st_rt0;
        p.dbg[wv * 8 + 4] = __builtin_amdgcn_s_memtime() - st_c0;
        p.dbg[wv * 8 + 5] = st_rt0;
        p.dbg[wv * 8 + 6] = rt1;
        p.dbg[wv * 8 + 7] = __builtin_amdgcn_s_getreg(/*HW_REG_XCC_ID*/ (20 << 0) | (0 << 6) | (3 << 11));
    }
#endif
    flush_bad<kDmaBad>(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Fixed length over 1524 B in segments of the wide kernel's cover (fcs_segw_kernel<WD>, WD 15..23,
// 26, 30, 32; host-selected by segment_wd()). fcs_segil_kernel's schedule (units of four frames, item r =
// segment r of the four, four DMA runs into 2 KiB parts of an 8 KiB slot, 12 waves) with
// fcs_wide_kernel<WD>'s lane windows (4 WD bytes every 4 WD - 4): C = wide_cover(WD) bytes per
// segment (1604 / 1860 B), so a frame takes ceil(L / C) items where fcs_segil_kernel takes
// ceil(L / 1524) (9216 B: 5 items of 30 words per lane against 7 of 24).
// The front segment of Lf = L - C (m - 1) bytes is the wide kernel's frame of length Lf (front lane
// cf, its zc leading bytes masked, INV[zc]; lanes past cf dropped; launch constants). In the other
// segments every lane masks its first word (the next lane's last) except lane 15, whose window
// starts at the segment start and whose chain starts from the frame's CRC state after the previous
// segment (the row XOR), as in fcs_segil_kernel.
// LDS: the wide kernel's 64 KiB table image, then 12 slots of 8 KiB (160 KiB).
// CPU model: tests/kernel_model.py model_segw_frame.
// ---------------------------------------------------------------------------------------------
template <int WD>
__global__ __launch_bounds__(kSegilThreads, 1) void fcs_segw_kernel(KParams p) {
    constexpr uint32_t kWin = wide_win(WD), kStep = wide_step(WD), kCov = wide_cover(WD);
    constexpr int CL0 = wide_cl0(WD), CL1 = WD - CL0, CLM = CL0 > CL1 ? CL0 : CL1;
    // a run (at most 15 bytes of alignment, the segment, the last window's extra dword) and the odd
    // runs' skew stay inside the run's 2 KiB part; two DMA rows of 64 pieces hold it
    static_assert(FCS_SEGIL_SKEW + 16 + kCov + 16 <= kSegilRunBytes && (kCov + 30) / 16 <= 128, "run part");
    __shared__ __attribute__((aligned(16))) uint8_t lds[kSegilLdsBytes];
    const int tid = threadIdx.x;
    stage_wide_tables<WD, 16, kSegilThreads>(p, lds, tid);
    init_bad<kWideBad>(lds);
    __syncthreads();

    // ---- frame geometry (wave-uniform) ----
    const uint32_t L = p.flen;
    const uint32_t m = (L + kCov - 1) / kCov;   // segments, >= 2
    const uint32_t Lf = L - kCov * (m - 1);     // front segment, 1 .. kCov

    const int lane = tid & 63;
    const int c = lane & 15;                    // window index back from the segment end
    const uint32_t q = (uint32_t)lane >> 4;     // quarter: frame 4 u + q of unit u
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *slot = lds + kDmaRing + (uint32_t)wave * kSegilSlotBytes;
    const uint8_t *run = slot + q * kSegilRunBytes + (q & 1u) * FCS_SEGIL_SKEW;
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    const uint32_t lanebase = kDmaHole + (uint32_t)(lane & 31) * 4u;

    // front segment: the wide kernel's front lane for length Lf (scalars but the lane tests)
    const uint32_t cf = (Lf - 1u) / kStep < 15u ? (Lf - 1u) / kStep : 15u;
    const uint32_t zc = kStep * cf + kWin - Lf;   // 0 .. kWin - 1
    const bool flive = (uint32_t)c <= cf, ffront = (uint32_t)c == cf;
    const uint32_t x0f = ffront ? lds_rd(lds, dma_hole(kWideInvHole + zc / 32u) + (zc % 32u) * 4u) : 0u;
    const uint32_t m0f = ffront ? (zc >= 4u ? 0u : (uint32_t)(0xFFFFFFFFull << (8u * zc))) : 0u;
    uint32_t keepf = ffront ? 0u : 0xFFFFFFFFu;
    asm volatile("" : "+v"(keepf));
    const uint32_t fgroups = (zc + 15u) / 16u;    // word groups of four holding masked front bytes
    // other segments: lane 15 takes the segment's first word whole
    const uint32_t m0n = c == 15 ? 0xFFFFFFFFu : 0u;

    const uint64_t n = p.n, units = (n + 3) >> 2;
    // chunk sizes as fcs_segil_kernel's
    constexpr uint32_t kSegilChunkItems = FCS_SEGIL_CMAX_ITEMS;
    const uint32_t cmax = m >= 4 ? (kSegilChunkItems / m > 32u ? 32u : (kSegilChunkItems / m < 1u ? 1u : kSegilChunkItems / m))
                                 : 64u / m;
    Dispenser D(p.ctr, units, (uint64_t)gridDim.x * kSegilWaves, (uint64_t)blockIdx.x * kSegilWaves + (uint64_t)wave,
                lane, 100, 1, cmax);
    D.align = 16;
    constexpr uint64_t kEnd = Dispenser::kEnd;
    auto seg_start = [&](uint64_t f, uint32_t r) {
        return p.base + f * p.stride + (r ? (uint64_t)Lf + (uint64_t)kCov * (r - 1) : 0ull);
    };
    auto issue = [&](uint64_t u, uint32_t r) {   // the item's four runs (wave-uniform control)
        const uint32_t len = r ? kCov : Lf;
#pragma unroll
        for (uint32_t qq = 0; qq < 4; qq++) {
            const uint64_t f = 4 * u + qq;
            if (f < n) {
                const uint64_t s0 = seg_start(f, r), a = s0 & ~15ull;
                const uint32_t pieces = (uint32_t)((((s0 + len) + 15) & ~15ull) - a) >> 4;
                segil_run(slot + qq * kSegilRunBytes + (qq & 1u) * FCS_SEGIL_SKEW, a, lane, pieces);
            }
        }
    };

    uint64_t u = D.first();
    uint32_t r = 0;
    if (u != kEnd) issue(u, 0);
    uint32_t acc = 0;     // this quarter's frame: CRC state after its segments so far
    uint32_t cbuf = 0;    // FCSs of the current run of units, lane 4 (unit & 15) + frame
    uint64_t cmask = 0;   // lanes of cbuf that hold one (wave-uniform)
    while (u != kEnd) {   // wave-uniform
        const uint64_t f = 4 * u + q;
        const uint64_t s0 = f < n ? seg_start(f, r) : 0ull;
        const uint32_t len = r ? kCov : Lf;
        // window start in the run: >= -(kWin - 1) for live lanes (the front lane's masked bytes may
        // lie before it); dropped front lanes read below the run, inside the LDS, and are discarded
        const int64_t x = (int64_t)(s0 & 15ull) + (int64_t)len - (int64_t)(kStep * (uint32_t)c) - (int64_t)kWin;
        const uint32_t ra = (uint32_t)x & 3u;
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's runs have landed
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(run + (x & ~3ll));
        uint32_t d[WD + 1];
#pragma unroll
        for (int i = 0; i <= WD; i++) d[i] = wp[i];
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA

        // ---- the next item: the next segment of the unit, or the dispenser's next unit ----
        uint64_t un = u;
        uint32_t rn = r + 1;
        if (rn == m) {
            un = D.next(u);
            rn = 0;
        }
        if (un != kEnd) issue(un, rn);

        // ---- this item ----
        uint32_t w[WD];
#pragma unroll
        for (int i = 0; i < WD; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], ra);
        uint32_t x0;
        bool live = true;
        if (r == 0) {
            w[0] &= m0f;
            // words 1.. of the front lane up to its zc bytes: groups of four below an opaque scalar
            // bound (hoisted group tests would each hold an SGPR pair)
            uint32_t gm = fgroups;
            asm volatile("" : "+s"(gm));
#pragma unroll
            for (int g = 0; g < (WD + 3) / 4; g++) {
                if ((uint32_t)g >= gm) break;
#pragma unroll
                for (int i = (4 * g > 1 ? 4 * g : 1); i < 4 * g + 4 && i < WD; i++) {
                    const int t = (int)zc - 4 * i;
                    const uint32_t mk = t >= 4 ? 0u : (uint32_t)(0xFFFFFFFFull << (8 * (t < 0 ? 0 : t)));
                    w[i] &= mk | keepf;
                }
            }
            x0 = x0f;
            live = flive;
        } else {
            w[0] &= m0n;
            x0 = c == 15 ? acc : 0u;
        }
        uint32_t xa = w[0] ^ x0, xb = w[CL0];
#pragma unroll
        for (int i = 0; i < CLM; i++) {
            if (i < CL0) xa = step4_l8(lds, xa, i < CL0 - 1 ? w[i + 1] : 0u, B, SEL);
            if (i < CL1) xb = step4_l8(lds, xb, i < CL1 - 1 ? w[CL0 + i + 1] : 0u, B, SEL);
        }
        const uint32_t mv = merge_shift_dma(lds, 0, xa, xb);
        uint32_t v = lane_shift_dma(lds, mv, lanebase);
        if (!live) v = 0u;
        acc = row_xor(v);
        if (r == m - 1) {   // results of consecutive units leave as one coalesced store
            const uint32_t k = (uint32_t)(u & 15u);
            const uint32_t vq = (uint32_t)__shfl((int)~acc, (lane & 3) * 16);
            if ((uint32_t)(lane >> 2) == k) cbuf = vq;
            const uint64_t f0 = 4 * u;
            cmask |= (f0 + 4 <= n ? 0xFull : ((1ull << (n - f0)) - 1ull)) << (4 * k);
            if (k == 15 || un != u + 1) {
                emit<kWideBad>(p, lds, (cmask >> lane) & 1ull, 4 * (u & ~15ull) + (uint64_t)lane, cbuf);
                cmask = 0;
            }
        }
        u = un;
        r = rn;
    }
    flush_bad<kWideBad>(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Variable-length frames: a lane's chunk loads and register value (fcs_flat_kernel below, and the
// segment loop of its frames over 1536 B).
// ---------------------------------------------------------------------------------------------
template <bool TINY>
__device__ __forceinline__ void issue_any(const KParams &p, int64_t cstart, bool need, Chunk &c) {
    LoadPriority lp;
    c.r = (uint32_t)cstart & 3u;
    const uint64_t a = need ? ((uint64_t)cstart & ~3ull) : p.lo4;
    c.dlead = 0;
    if (TINY) {
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q <= kChunkWords; q++) {
            const uint64_t ad = a + 4 * q;
            d[q] = (need && ad >= p.lo4 && ad + 4 <= p.hi4) ? gload<uint32_t>(ad) : 0u;
        }
#pragma unroll
        for (int g = 0; g < 6; g++) c.x[g] = u32x4a4{d[4 * g], d[4 * g + 1], d[4 * g + 2], d[4 * g + 3]};
        c.x6 = d[kChunkWords];
        return;
    }
    uint64_t ab = a;
    if (__any(a < p.lo4)) {
        c.dlead = a < p.lo4 ? (int)((p.lo4 - a) >> 2) : 0;
        ab = a < p.lo4 ? p.lo4 : a;
    }
#pragma unroll
    for (int q = 0; q < 6; q++) c.x[q] = gload<u32x4a4>(ab + 16 * q);
    c.x6 = gload<uint32_t>(ab + ((c.r || c.dlead) ? 96 : 92));
}

// Register value of one chunk (realigned, bytes before the frame start masked, x0 injected),
// before the lane shift: A_48(chain(words 0..11)) ^ chain(words 12..23).
// zb: this lane's claim on the masking (zr if its value is used, 0 if the caller discards it): the
// wave masks 16-byte groups of words only up to its largest claim (IMIX items: 32 bytes, not 96).
template <bool TINY>
__device__ __forceinline__ uint32_t chunk_value(const uint8_t *lds, const Chunk &c, int zr, int zb, uint32_t x0,
                                                uint32_t base0, uint32_t base1) {
    uint32_t d[kChunkWords + 1];
#pragma unroll
    for (int q = 0; q < 6; q++) {
        d[4 * q] = c.x[q].x;
        d[4 * q + 1] = c.x[q].y;
        d[4 * q + 2] = c.x[q].z;
        d[4 * q + 3] = c.x[q].w;
    }
    d[kChunkWords] = c.x6;
    if (!TINY && __any(c.dlead)) shift_up(d, c.dlead);
    uint32_t w[kChunkWords];
#pragma unroll
    for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], c.r);
#ifdef FCS_MASK_ALL   // measurement-only build: every word masked whenever any lane has a front
    if (__any(zr > 0)) {
#pragma unroll
        for (int i = 0; i < kChunkWords; i++) {
            int t = zr - 4 * i;
            t = t < 0 ? 0 : (t > 4 ? 4 : t);
            w[i] &= (uint32_t)(0xFFFFFFFFull << (8 * t));
        }
    }
#else
    const int zr8 = 8 * zr;
#pragma unroll
    for (int g = 0; g < kChunkWords / 4; g++) {
        if (!__any(zb > 16 * g)) break;
#pragma unroll
        for (int i = 4 * g; i < 4 * g + 4; i++) {
            w[i] = clear_low_bits(w[i], zr8 - 32 * i);
        }
    }
#endif
    uint32_t xa = x0 ^ w[0], xb = w[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        xa = step4(lds, xa, i < 11 ? w[i + 1] : 0u, base0, base1);
        xb = step4(lds, xb, i < 11 ? w[13 + i] : 0u, base0, base1);
    }
    return uniform_shift<kLdsH48>(lds, xa, xb);
}

__device__ __forceinline__ int clamp_zr(int64_t z) {
    return z < -1 ? -1 : (z > kChunkBytes ? kChunkBytes : (int)z);
}

// ---------------------------------------------------------------------------------------------
// Variable-length frames, flat chunk stream (fcs_flat_kernel).
// A wave owns windows of 64 consecutive frames. Every frame of at most 1536 bytes needs
// k = ceil(len / 96) chunks (an empty frame one dummy chunk); the window's chunks are numbered
// frame by frame (exclusive prefix P over the window) and dealt to the lanes 64 at a time, so
// every lane of an item carries a real chunk whatever the mix of lengths (a 576-B frame takes
// 6 lanes, not 8; small, medium and full frames pack without gaps). Per item a lane finds its
// frame from the frame-start marks (one LDS byte per chunk slot, a ballot and a popcount),
// computes its chunk's register exactly as the other kernels do, shifts it by A_{96c} for its
// chunk index c (tables indexed by c, stride 4 mod 64 banks) and XORs it into the frame's LDS
// accumulator (ds_xor). At the end of the window lane i stores frame i's FCS: one coalesced
// store per window. Frames over 1536 bytes take the segment loop of fcs_var_kernel.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t chunk_shift(const uint8_t *lds, uint32_t s, uint32_t c) {
    uint32_t r[8];
    const uint32_t base = kLdsFlat + c * kFlatStride;
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint32_t sh = (4 * t >= 2) ? (s >> (4 * t - 2)) : (s << 2);
        r[t] = lds_rd(lds, base + (sh & 0x3Cu) + t * 64);
    }
    return xor9(r, 0u);
}

template <bool TINY>
__global__ __launch_bounds__(kWgThreads, 1) void fcs_flat_kernel(KParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kLdsBytes];
    // After fcs_stream_kernel (p.ulist set): only the units it listed, 8 windows each; none -> done.
    uint64_t nwin = (p.n + 63) >> 6;
    if (p.ulist != nullptr) {
        const uint32_t listed = (uint32_t)__builtin_amdgcn_readfirstlane((int)*p.ucount);
        if (blockIdx.x == 0 && threadIdx.x == 0 && p.listed_out) *p.listed_out = listed;   // fcs_debug_stream_listed
        nwin = (uint64_t)listed * (kStUnitFrames / 64);
        if (nwin == 0) return;
    }
    stage_tables_flat(p, lds);
    init_bad(lds);

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int j = lane & (kGroup - 1);
    uint32_t base0, base1;
    table_bases(lane, base0, base1);
    uint32_t *acc = reinterpret_cast<uint32_t *>(lds + kLdsWave + wave * kLdsWaveBytes);   // 64 frames
    uint8_t *mark = lds + kLdsFlatMark + wave * 64;
    uint8_t *list = lds + kLdsFlatList + wave * 64;
    acc[lane] = 0u;
    mark[lane] = 0;
    // windows of 64 frames from the dispenser (dynamic chunks of up to 16 windows when p.ctr is set)
    Dispenser D(p.ctr, nwin, (uint64_t)gridDim.x * (kWgThreads / 64),
                (uint64_t)blockIdx.x * (kWgThreads / 64) + (uint64_t)wave, lane, 100, 1, FCS_FLAT_CHUNK_MAX);
    for (uint64_t wi = D.first(); wi != Dispenser::kEnd; wi = D.next(wi)) {
        constexpr uint32_t kUw = kStUnitFrames / 64;   // windows per listed unit
        const uint64_t win = p.ulist ? (uint64_t)p.ulist[wi / kUw] * kUw + wi % kUw : wi;
        const uint64_t w0 = win * 64;
        // ---- window metadata: lane i <-> frame w0 + i ----
        const uint64_t f = w0 + lane;
        const bool act = f < p.n;
        const uint32_t L = act ? (p.len ? p.len[f] : p.flen) : 0u;   // len == null: fixed length
        const uint64_t E = act ? p.base + (p.off ? p.off[f] : f * p.stride) + L : p.lo4;
        const bool multi = act && L > (uint32_t)kSegBytes;
        const uint32_t k = (!act || multi) ? 0u : (L ? (L + kChunkBytes - 1) / kChunkBytes : 1u);
        uint32_t incl = k;   // inclusive prefix over the window
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= d) incl += y;
        }
        const uint32_t P = incl - k;
        const uint32_t PL = P | ((L > 0xFFFFu ? 0xFFFFu : L) << 16);   // see deal()
        const uint32_t K = (uint32_t)__shfl((int)incl, 63);
        const uint64_t fmask = __ballot(k != 0);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(fmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)fmask, 0u));
        if (k) list[rank] = (uint8_t)lane;
        wave_lds_sync();
        const uint32_t Elo = (uint32_t)E, Ehi = (uint32_t)(E >> 32);
#ifndef FCS_FLAT_NO_SHORTCUTS   // measurement-only: always the list read and four bpermutes
        // common windows: no frame over 1536 B (the frames with chunks are lanes 0, 1, ..., so a
        // chunk's frame rank is its frame's lane: no list read), and all frame ends in one 4 GiB
        // page of addresses (the high word is shared: one bpermute fewer)
        const bool dense = __ballot(multi) == 0;
        const uint32_t Ehi0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)Ehi);
        const bool onehi = __ballot(Ehi != Ehi0) == 0;
#else
        const bool dense = false, onehi = false;
        const uint32_t Ehi0 = 0;
#endif

        // one item = 64 chunks; resolve lane -> (frame, chunk) and issue its loads
        struct FlatItem {
            Chunk ch;
            int src, zr;
            uint32_t c;
            bool valid;
            int64_t cstart;
        };
        auto deal = [&](uint32_t g0, uint32_t tag, FlatItem &it) {
            // frame starts inside this item: mark their slot, then lane g finds its frame's rank
            // as (frames started before the item) + (marks at or below g) - 1
            if (k && P >= g0 && P < g0 + 64) mark[P - g0] = (uint8_t)tag;
            wave_lds_sync();
            const uint32_t before = (uint32_t)__popcll(__ballot(k && P < g0));
            const uint64_t M = __ballot(mark[lane] == (uint8_t)tag);
            const uint32_t g = g0 + (uint32_t)lane;
            it.valid = g < K;
            const uint32_t rk = before + (uint32_t)__popcll(M & ((2ull << lane) - 1ull)) - 1u;
            it.src = it.valid ? (dense ? (int)(rk & 63u) : (int)list[rk & 63u]) : 0;
            const uint32_t Eghi = onehi ? Ehi0 : (uint32_t)__shfl((int)Ehi, it.src);
            const uint64_t Eg = ((uint64_t)Eghi << 32) | (uint32_t)__shfl((int)Elo, it.src);
            // one shuffle for both: a frame that holds chunks is at most 1536 B, a prefix at most 1024
            // (two shuffles measured the same: IMIX 5036 vs 5041 GB/s, one process)
            const uint32_t PLg = (uint32_t)__shfl((int)PL, it.src);
            const uint32_t Lg = PLg >> 16, Pg = PLg & 0xFFFFu;
            it.c = it.valid ? g - Pg : 0u;   // chunk index back from the frame end
            it.cstart = (int64_t)Eg - (int64_t)kChunkBytes * (int64_t)(it.c + 1);
            // bytes of the window before the frame start: (Eg - Lg) - cstart
            it.zr = it.valid ? clamp_zr((int64_t)kChunkBytes * (int64_t)(it.c + 1) - (int64_t)Lg) : kChunkBytes;
        };
        auto issue = [&](FlatItem &it) { issue_any<TINY>(p, it.cstart, it.valid && it.zr < kChunkBytes, it.ch); };
        auto prep = [&](uint32_t g0, uint32_t tag, FlatItem &it) {
            deal(g0, tag, it);
            issue(it);
        };
        auto finish = [&](const FlatItem &it) {
#ifdef FCS_FLAT_NOCRC   // measurement-only build: loads and dealing without the CRC work (wrong FCS)
            uint32_t v = it.ch.x6 ^ it.c;
#pragma unroll
            for (int q = 0; q < 6; q++) v ^= it.ch.x[q].x ^ it.ch.x[q].y ^ it.ch.x[q].z ^ it.ch.x[q].w;
#else
            // lanes past the window's chunks and the dummy chunk of an empty frame (zr = 96) are discarded
            const uint32_t own = chunk_value<TINY>(lds, it.ch, it.zr, it.zr < kChunkBytes ? it.zr : 0,
                                                   it.valid ? inv_start(lds, it.zr) : 0u, base0, base1);
            const uint32_t v = chunk_shift(lds, own, it.c & 15u);
#endif
            if (it.valid && v) atomicXor(&acc[it.src], v);
        };
        for (uint32_t g0 = 0, tag = 1; g0 < K; g0 += 64, tag++) {
            FlatItem it;
            prep(g0, tag, it);
            finish(it);
        }

        // ---- frames over 1536 B: 16 lanes each, 4 per item, segment by segment ----
        const uint64_t xmask = __ballot(multi);
        const uint32_t nx = (uint32_t)__popcll(xmask);
        if (nx) {
            const uint32_t rx = __builtin_amdgcn_mbcnt_hi((uint32_t)(xmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)xmask, 0u));
            if (multi) mark[rx] = (uint8_t)lane;   // the marks are free again: reuse them as the multi list
            wave_lds_sync();
            for (uint32_t t = 0; t < nx; t += 4) {
                const uint32_t rnk = t + (uint32_t)(lane >> 4);
                const bool valid = rnk < nx;
                const int src = valid ? (int)mark[rnk] : 0;
                const uint64_t Eq = ((uint64_t)(uint32_t)__shfl((int)Ehi, src) << 32) | (uint32_t)__shfl((int)Elo, src);
                const uint32_t Lq = (uint32_t)__shfl((int)L, src);
                const uint32_t m = valid ? (Lq + (kSegBytes - 1)) / kSegBytes : 0u;
                uint32_t s = 0;
                for (uint32_t q = 0; __any(q < m); q++) {
                    const bool on = q < m;
                    const int64_t cstart = (int64_t)Eq - (int64_t)kSegBytes * (int64_t)(m - 1 - q) -
                                           (int64_t)kChunkBytes * (j + 1);
                    const int zr = (on && q == 0) ? clamp_zr((int64_t)(Eq - Lq) - cstart) : (on ? -1 : kChunkBytes);
                    Chunk cc;
                    issue_any<TINY>(p, cstart, on && zr < kChunkBytes, cc);
                    const uint32_t r = chunk_value<TINY>(lds, cc, zr, on ? zr : 0, (on && q == 0) ? inv_start(lds, zr) : 0u,
                                                         base0, base1);
                    s = on ? (q == 0 ? r : uniform_shift<kLdsJump>(lds, s, r)) : s;
                }
                const uint32_t v = row_xor(chunk_shift(lds, s, (uint32_t)j));
                if (valid && j == 15) acc[src] = v;
            }
            if (multi) mark[rx] = 0;
        }

        // ---- one coalesced store per window; clear the window state ----
        wave_lds_sync();
        const uint32_t a = acc[lane];
        emit(p, lds, act, f, L ? ~a : 0u);
        acc[lane] = 0u;
        mark[lane] = 0;
    }
    flush_bad(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Short fixed-length frames, one lane per frame (fcs_short_kernel<W>; host-selected by
// short_wd(): frames of 1..64 B on W = 16, 65..96 B on W = 24, 97..128 B on W = 32, large batches,
// any stride).
// The flat chunk stream (fcs_flat_kernel) spends a 96-B chunk on a 64-B frame: a 24-word chain of
// which 8 words are masked, the dealing of chunks to lanes, a chunk shift and an LDS atomic. With
// the length fixed none of that is needed: lane l of a wave's item takes frame 64 item + l, loads
// the W dwords ending at the frame end (plus the realignment dword) straight into registers, masks
// the zc = 4 W - len bytes before the frame start (zc is a launch constant: scalar masks) and runs
// two chains of W / 2 words from INV[zc], merged with A_{2 W}. Its FCS leaves in one coalesced
// 256-B store per item. Items come from the dispenser (dynamic for large batches).
// LDS: the 64 KiB table image of fcs_wide_kernel (slice tables; holes 128..131 the merge A_{2 W},
// 132..135 INV[0..127]); no slots. CPU model: tests/kernel_model.py model_short_frame.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kShortLdsBytes = kDmaRing;   // the table image only
template <int W>
__global__ __launch_bounds__(kWgThreads, 1) void fcs_short_kernel(KParams p) {
    static_assert(W % 8 == 0 && W >= 8 && W <= 32, "two chains of an even word count; merge A_{2 W} = A_{8 (W / 4)}");
    __shared__ __attribute__((aligned(16))) uint8_t lds[kShortLdsBytes];
    const int tid = threadIdx.x;
    for (int i = tid; i < 2048; i += kWgThreads) {   // slice tables as fcs_dma_kernel
        const uint32_t v = p.blob[kBlobSlice + 256 * (3 - ((i & 7) >> 1)) + (i >> 3)];
        u32x4 vv = {v, v, v, v};
        *reinterpret_cast<u32x4 *>(lds + (uint32_t)(i >> 3) * 256u + (uint32_t)(i & 7) * 16u) = vv;
    }
    for (int i = tid; i < 128; i += kWgThreads) {   // the chain merge A_{2 W}
        const int t = (i >> 4) & 7, e = i & 15;
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kWideMergeHole + (uint32_t)(t >> 1)) + 64u * (uint32_t)(t & 1) +
                                      4u * (uint32_t)e) = p.blob[kBlobMerge + (W / 4 - 1) * 128 + i];
    }
    for (int i = tid; i < (int)kWideWin; i += kWgThreads)
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kWideInvHole + (uint32_t)i / 32u) + (uint32_t)(i % 32) * 4u) =
            p.blob[kBlobInvWide + i];
    init_bad<kWideBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    // launch constants: the masked bytes before the frame start and the chain's start value
    const uint32_t zc = 4u * (uint32_t)W - p.flen;   // 0 .. 4 W - 1 (host: 1 <= len <= 4 W)
    const uint32_t x0 = lds_rd(lds, dma_hole(kWideInvHole + zc / 32u) + (zc % 32u) * 4u);

    constexpr uint64_t kEnd = Dispenser::kEnd;
    constexpr int kWaves = kWgThreads / 64;
    const uint64_t n = p.n;
    Dispenser D(p.ctr, (n + 63) >> 6, (uint64_t)gridDim.x * kWaves, (uint64_t)blockIdx.x * kWaves + wave, lane,
                100, 1, 16);
    // one item's window loads (issued one item ahead of its CRC work: two register sets, ping-pong)
    struct Win {
        uint32_t d[W + 1];
        uint32_t r;
    };
    auto load = [&](uint64_t it, Win &x) {
        const uint64_t f = 64 * it + (uint64_t)lane;
        // the window [E - 4 W, E) of this lane's frame; lanes past n read the first frame's
        const uint64_t E = p.base + (f < n ? f : 0ull) * p.stride + p.flen;
        const uint64_t a = (E - 4u * (uint32_t)W) & ~3ull;   // may lie before the frame (masked) and before lo4
        x.r = (uint32_t)E & 3u;
        if (__any(a < p.lo4)) {   // a window reaching before the arena's first dword: guarded loads
#pragma unroll
            for (int q = 0; q <= W; q++) {
                const uint64_t ad = a + 4u * (uint32_t)q;
                x.d[q] = (ad >= p.lo4 && ad + 4 <= p.hi4) ? gload<uint32_t>(ad) : 0u;
            }
        } else {
            LoadPriority lp;
#pragma unroll
            for (int q = 0; q < W / 4; q++) {
                const u32x4a4 v = gload<u32x4a4>(a + 16u * (uint32_t)q);
                x.d[4 * q] = v.x;
                x.d[4 * q + 1] = v.y;
                x.d[4 * q + 2] = v.z;
                x.d[4 * q + 3] = v.w;
            }
            // dword W matters only when r != 0; then it ends at ceil4(E) <= hi4 (else re-read W - 1)
            x.d[W] = gload<uint32_t>(a + (x.r ? 4u * (uint32_t)W : 4u * (uint32_t)(W - 1)));
        }
    };
    auto crc = [&](uint64_t it, const Win &x) {
        const uint64_t f = 64 * it + (uint64_t)lane;
        uint32_t w[W];
#pragma unroll
        for (int i = 0; i < W; i++) w[i] = __builtin_amdgcn_alignbyte(x.d[i + 1], x.d[i], x.r);
#pragma unroll
        for (int i = 0; i < W; i++) {   // the zc bytes before the frame start go (scalar masks)
            const int t = (int)zc - 4 * i;
            w[i] &= t >= 4 ? 0u : (t <= 0 ? 0xFFFFFFFFu : (uint32_t)(0xFFFFFFFFull << (8 * t)));
        }
        constexpr int CL = W / 2;
        uint32_t xa = w[0] ^ x0, xb = w[CL];
#pragma unroll
        for (int i = 0; i < CL; i++) {
            xa = step4_l8(lds, xa, i < CL - 1 ? w[i + 1] : 0u, B, SEL);
            xb = step4_l8(lds, xb, i < CL - 1 ? w[CL + i + 1] : 0u, B, SEL);
        }
        const uint32_t v = merge_shift_dma(lds, 0, xa, xb);
        emit<kWideBad>(p, lds, f < n, f, ~v);
    };
#ifdef FCS_SHORT_NO_PIPE   // measurement-only: each item's loads right before its CRC work
    constexpr bool kPipe = false;
#else
    constexpr bool kPipe = W <= 24;   // two 33-dword register sets at W = 32 spill (W = 24: 103 VGPRs)
#endif
    if constexpr (!kPipe) {
        for (uint64_t it = D.first(); it != kEnd; it = D.next(it)) {
            Win x;
            load(it, x);
            crc(it, x);
        }
    } else {
    Win xa, xb;
    uint64_t it = D.first();
    if (it != kEnd) load(it, xa);
    while (it != kEnd) {   // wave-uniform
        const uint64_t i1 = D.next(it);
        if (i1 != kEnd) load(i1, xb);
        crc(it, xa);
        if (i1 == kEnd) break;
        const uint64_t i2 = D.next(i1);
        if (i2 != kEnd) load(i2, xa);
        crc(i1, xb);
        it = i2;
    }
    }
    flush_bad<kWideBad>(p, lds);
}

// ---------------------------------------------------------------------------------------------
// Variable-length frames, arena stream (fcs_stream_kernel): batches with offsets, windowed size.
// CPU model of the decomposition: tests/stream_model.py.
// The dispenser hands out units of kStUnitFrames frames. A unit whose frames are packed
// (off[i + 1] == off[i] + len[i]) and 64..1536 B long is taken here; any other unit is listed
// in p.ulist for fcs_flat_kernel, launched right after on the same stream.
// A unit's bytes are walked in 4 KiB items at fixed arena positions (the first item at the 128-B
// line below the unit's first frame, so items share no line and every row is non-temporal): one
// coalesced LDS-DMA per item (four 1 KiB rows from one address register), issued while the previous
// item is computed, no dealing. Lane l's chunk is the
// item's bytes [64 l, 64 l + 64); its 16-B pieces sit in LDS swizzled (piece m of chunk l at
// 64 l + 16 ((m + l / 4) mod 4)), so the four ds_read_b128 of a chunk are conflict-free without
// padding. Its chain L runs over all 16 words from register 0.
// A frame starts in at most one place of a chunk (frames >= 64 B); there the lane takes a tap of
// its chain, T' = A_4(s_k ^ (w_k & the k-th word's bytes before the boundary)), s_k the chain
// after k = sigma / 4 words, and records it for the frame starting there (it is also the end tap
// of the frame before). Every chunk goes to the frame holding its last byte, shifted by whole
// chunks to the chunk holding that frame's end, A_{64 j}(L) with j = le - l - 1; the lanes of one
// frame are summed by a wave-wide XOR scan, and the lane ending the frame's run of lanes adds the
// run's sum to the frame's LDS accumulator (one plain read-modify-write per frame and item: an LDS
// atomic here made the compiler wait for the next item's DMA, vmcnt(0), before it). Once 64
// frames have ended, one pass closes them, a frame per lane:
//   acc ^= A_{64 (le - ls - 1)}(A_{4 (15 - k_s)}(T'_s) ^ A_{64 - sigma_s}(~0))   (its start)
//   R(~0, frame) = A_{r_e - 4}(T'_e ^ A_{4 (k_e + 1)}(acc)),  sigma_e = 4 k_e + r_e   (its end)
// and stores the 64 FCSs as one 256-B row. The frames' ends and lengths stay in registers from
// the unit's packed check (one word per frame), so no global load waits inside the item loop.
// LDS (144 KiB): the 32 KiB slice tables of fcs_dma_kernel with, in the row holes, A_{64 j}
// (j = 0..23), A_{4 i} (i = 0..16), A_{-d} (d = 1..4), K1[sigma] = A_{64 - sigma}(~0), the
// chunk marks of every wave and the verify counters; 16 slots of 4 KiB; per wave accumulators
// and start taps of 128 frames.
// ---------------------------------------------------------------------------------------------
constexpr uint32_t kStChunk = 64;
constexpr uint32_t kStItem = 64 * kStChunk;
constexpr uint32_t kStSlotBytes = kStItem;
constexpr int kStWaves = kWgThreads / 64;
constexpr uint32_t kStHoleChunk = 0;                                   // A_{64 j}: 4 holes each
constexpr uint32_t kStHoleWord = kStHoleChunk + 4 * kStChunkTabs;     // A_{4 i}
constexpr uint32_t kStHoleInv = kStHoleWord + 4 * kStWordTabs;        // A_{-d}
constexpr uint32_t kStHoleK1 = kStHoleInv + 4 * kStInvTabs;           // 2 holes
constexpr uint32_t kStHoleMark = kStHoleK1 + 2;                       // 2 holes per wave
constexpr uint32_t kStBad = dma_hole(kStHoleMark + 2 * 16);           // 16 x 8 B
static_assert(kStHoleMark + 2 * 16 + 1 <= 256, "holes");
static_assert(kStWaves <= 16, "marks and counters for 16 waves");
constexpr uint32_t kStSlots = 65536;
constexpr uint32_t kStRings = kStSlots + 16 * kStSlotBytes;           // per wave: acc[128], tap[128]
constexpr uint32_t kStLdsBytes = kStRings + 16 * 1024;
static_assert(kStLdsBytes <= 163840, "LDS per CU");
constexpr uint32_t kMarkStart = 1u << 31, kMarkEnd = 1u << 30;
// A frame's end (relative to the unit's first item, which starts at most 127 B before the unit)
// and length in one word: end << 11 | len (ends < 2^20: 512 frames of at most 1536 B; lengths < 2^11).
constexpr uint32_t kStLenBits = 11;
static_assert(kStUnitFrames * kStMaxLen + 128 < (1u << (32 - kStLenBits)) && kStMaxLen < (1u << kStLenBits), "packing");
// FCS_STAMPS (measurement-only): per-wave s_memtime sums of the item's phases (tools/stamps_stream.py)
#ifdef FCS_STAMPS
#define ST_T(v)                              \
    __builtin_amdgcn_sched_barrier(0);       \
    const uint64_t v = __builtin_amdgcn_s_memtime(); \
    __builtin_amdgcn_sched_barrier(0);
#else
#define ST_T(v)
#endif
#ifndef FCS_ST_CHAINS   // independent chains per 64-B chunk (1 or 2; measurement override)
#define FCS_ST_CHAINS 1
#endif
#ifndef FCS_ST_AUX   // cache policy of the item DMA's middle rows (measurement-only override)
#define FCS_ST_AUX 2
#endif
// Items at 128-B line boundaries: a unit's first item starts at the line below its first frame (not
// before the arena's first 16-B piece), so consecutive items share no line and every row is
// non-temporal (round 5, tools/ab.py --imix, one process, two boxes: +0.95 % and +1.0 % against
// 16-B-aligned items whose first and last rows took the default policy to keep the line they shared
// in L2). Measurement-only: FCS_ST_ALIGN16 restores the 16-B items, FCS_ST_EDGE_AUX their policy.
#ifndef FCS_ST_EDGE_AUX
#ifdef FCS_ST_ALIGN16
#define FCS_ST_EDGE_AUX 0
#else
#define FCS_ST_EDGE_AUX FCS_ST_AUX
#endif
#endif

// A_n(s) ^ extra from the nibble table at holes h .. h + 3 (h = 4 q for table q; h may differ per
// lane). Nibble t sits in hole h + t / 2, in the half (t + q) & 1 of its 32 banks: lanes shifting by
// tables of both parities in one lookup spread over all 32 banks instead of 16 (the chunk shifts'
// table index is data-dependent, so a lookup mixes tables; same-address reads broadcast).
#ifndef FCS_ST_NOSKEW
constexpr uint32_t kStSkew = 1;
#else   // measurement-only: every table's even nibbles in the low half (round-3 first layout)
constexpr uint32_t kStSkew = 0;
#endif
__device__ __forceinline__ uint32_t hole_shift(const uint8_t *lds, uint32_t s, uint32_t h, uint32_t extra) {
    uint32_t r[8];
    const uint32_t base = h * 256u + kDmaHole;
    const uint32_t ev = 64u * ((h >> 2) & kStSkew), od = 64u - ev;   // byte offset of the even / odd nibbles' half
#pragma unroll
    for (int t = 0; t < 8; t++) {
        const uint32_t sh = (4 * t >= 2) ? (s >> (4 * t - 2)) : (s << 2);
        r[t] = lds_rd(lds, base + 256u * (uint32_t)(t >> 1) + ((t & 1) ? od : ev) + (sh & 0x3Cu));
    }
    return xor9(r, extra);
}

// Inclusive XOR scan over the 64 lanes (row shifts within each 16-lane row, then the row
// broadcasts of gfx9 DPP).
__device__ __forceinline__ uint32_t wave_xor_scan(uint32_t v) {
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);   // row_shr:1
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);   // row_shr:2
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);   // row_shr:4
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);   // row_shr:8
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15 -> rows 1, 3
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

__device__ __forceinline__ void stage_stream_tables(const KParams &p, uint8_t *lds, int tid) {
    for (int i = tid; i < 2048; i += kWgThreads) {   // slice tables as fcs_dma_kernel
        const uint32_t v = p.blob[kBlobSlice + 256 * (3 - ((i & 7) >> 1)) + (i >> 3)];
        u32x4 vv = {v, v, v, v};
        *reinterpret_cast<u32x4 *>(lds + (uint32_t)(i >> 3) * 256u + (uint32_t)(i & 7) * 16u) = vv;
    }
    for (int i = tid; i < (kStChunkTabs + kStWordTabs + kStInvTabs) * 128; i += kWgThreads) {
        const uint32_t q = (uint32_t)i >> 7, t = ((uint32_t)i >> 4) & 7u, e = (uint32_t)i & 15u;
        *reinterpret_cast<uint32_t *>(lds + dma_hole(4u * q + (t >> 1)) + 64u * ((t + (q & kStSkew)) & 1u) + 4u * e) =
            p.blob[kBlobStream + i];
    }
    for (int i = tid; i < 64; i += kWgThreads)
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kStHoleK1 + (uint32_t)i / 32u) + ((uint32_t)i % 32u) * 4u) =
            p.blob[kBlobStreamK1 + i];
    for (int i = tid; i < 2 * 16 * 32; i += kWgThreads)   // marks: empty
        *reinterpret_cast<uint32_t *>(lds + dma_hole(kStHoleMark + (uint32_t)i / 32u) + ((uint32_t)i % 32u) * 4u) = 0u;
    for (int i = tid; i < 16 * 256; i += kWgThreads) reinterpret_cast<uint32_t *>(lds + kStRings)[i] = 0u;
}

// A unit of the arena-stream kernels: frames f0 .. f0 + nf - 1, batch q of 64 in S[q] (arena
// offsets) and Ln[q] (lengths), lane = frame within the batch. True in the lanes that find the unit
// unfit for the stream walk: a length outside 64..1536, or a frame not starting where the one
// before it ends (the caller hands such units to fcs_flat_kernel).
template <int kQ>
__device__ __forceinline__ bool unit_unpacked(const KParams &p, uint64_t f0, uint32_t nf, int lane, uint64_t (&S)[kQ],
                                              uint32_t (&Ln)[kQ]) {
#pragma unroll
    for (int q = 0; q < kQ; q++) {
        const uint32_t g = 64u * (uint32_t)q + (uint32_t)lane;
        S[q] = g < nf ? p.off[f0 + g] : 0ull;
        Ln[q] = g < nf ? p.len[f0 + g] : kStMinLen;
    }
    bool bad = false;
#pragma unroll
    for (int q = 0; q < kQ; q++) {
        const uint32_t g = 64u * (uint32_t)q + (uint32_t)lane;
        bad |= Ln[q] < kStMinLen || Ln[q] > kStMaxLen;
        // the next frame's start: lane + 1 of this batch, or lane 0 of the next one
        uint32_t nlo = (uint32_t)__shfl_down((int)(uint32_t)S[q], 1), nhi = (uint32_t)__shfl_down((int)(uint32_t)(S[q] >> 32), 1);
        if (q + 1 < kQ) {
            const uint32_t blo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)S[q + 1]);
            const uint32_t bhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(S[q + 1] >> 32));
            if (lane == 63) {
                nlo = blo;
                nhi = bhi;
            }
        }
        const uint64_t ns = ((uint64_t)nhi << 32) | nlo;
        bad |= g + 1 < nf && ns != S[q] + Ln[q];
    }
    return bad;
}

// LOAD: the measurement form behind fcs_stream_load_dev: the same units, unit
// check, items, slot DMA and schedule, but no marks, chain, contributions or closes; each lane only
// XORs its chunk's words (the stream kernel's own load ceiling).
template <bool LOAD>
__global__ __launch_bounds__(kWgThreads, 1) void fcs_stream_kernel(KParams p) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[kStLdsBytes];
    const int tid = threadIdx.x;
    stage_stream_tables(p, lds, tid);
    init_bad<kStBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    uint8_t *slot = lds + kStSlots + wave * kStSlotBytes;
    uint32_t *acc = reinterpret_cast<uint32_t *>(lds + kStRings + wave * 1024u);   // per frame (mod 128)
    uint32_t *tap = acc + 128;                                                      // start tap per frame
    const uint32_t mark_lane = dma_hole(kStHoleMark + 2u * wave + ((uint32_t)lane >> 5)) + ((uint32_t)lane & 31u) * 4u;
    auto mark_at = [&](uint32_t c) {
        return reinterpret_cast<uint32_t *>(lds + dma_hole(kStHoleMark + 2u * wave + (c >> 5)) + (c & 31u) * 4u);
    };
    auto k1_of = [&](uint32_t sg) { return lds_rd(lds, dma_hole(kStHoleK1 + sg / 32u) + (sg % 32u) * 4u); };
    // item DMA: row q, lane i moves the 16-B piece that sits at slot byte 1024 q + 16 i: chunk
    // l = 16 q + i / 4, piece m = (i - i / 16) mod 4 (the swizzle), arena byte X + 1024 q + goff
    const uint32_t goff = 64u * ((uint32_t)lane >> 2) + 16u * (((uint32_t)lane - ((uint32_t)lane >> 4)) & 3u);
    const uint64_t hi16 = (p.hi4 + 15) & ~15ull;
    auto dma_item = [&](uint64_t X) {
        typedef __attribute__((address_space(3))) void lds_void;
        const uint64_t a = X + goff;
        lds_void *ls = (lds_void *)slot;
        if (X + kStItem <= hi16) {   // wave-uniform: the whole item lies inside the arena's 16-B pieces
            // first and last rows at the default policy (lines shared with the neighbouring items)
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 0, FCS_ST_EDGE_AUX);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 1024, FCS_ST_AUX);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 2048, FCS_ST_AUX);
            __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 3072, FCS_ST_EDGE_AUX);
        } else {
            if (a < hi16) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 0, FCS_ST_EDGE_AUX);
            if (a + 1024 < hi16) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 1024, FCS_ST_AUX);
            if (a + 2048 < hi16) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 2048, FCS_ST_AUX);
            if (a + 3072 < hi16) __builtin_amdgcn_global_load_lds(reinterpret_cast<const void *>(a), ls, 16, 3072, FCS_ST_EDGE_AUX);
        }
    };
    // piece m of this lane's chunk in the slot (loop invariants)
    const uint32_t cbase = 64u * (uint32_t)lane, sw = ((uint32_t)lane >> 2) & 3u;
    const u32x4 *pc[4] = {reinterpret_cast<const u32x4 *>(slot + cbase + 16u * ((0u + sw) & 3u)),
                          reinterpret_cast<const u32x4 *>(slot + cbase + 16u * ((1u + sw) & 3u)),
                          reinterpret_cast<const u32x4 *>(slot + cbase + 16u * ((2u + sw) & 3u)),
                          reinterpret_cast<const u32x4 *>(slot + cbase + 16u * ((3u + sw) & 3u))};
    constexpr int kQ = (int)(kStUnitFrames / 64);
    constexpr uint32_t kLenMask = (1u << kStLenBits) - 1u;

    constexpr uint64_t kEnd = Dispenser::kEnd;
    const uint64_t units = (p.n + kStUnitFrames - 1) / kStUnitFrames;
#ifdef FCS_STAMPS   // [0] unit prologue [1] marks [2] slot wait [3] words + DMA + chain [4] rest [5] items [6] units [7] all
    uint64_t sts[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t st_begin = __builtin_amdgcn_s_memtime();
#endif
    Dispenser D(p.ctr, units, (uint64_t)gridDim.x * kStWaves, (uint64_t)blockIdx.x * kStWaves + wave, lane, 100, 1, 8);
    uint32_t lx = 0;   // LOAD only: the XOR of every word this lane read
#if defined(FCS_ST_PROBE_LDS) || defined(FCS_ST_PROBE_VALU)
    uint32_t probe = 0;   // measurement-only sensitivity probes (kept live below)
#endif
    for (uint64_t u = D.first(); u != kEnd; u = D.next(u)) {
        ST_T(tu0)
        const uint64_t f0 = u * kStUnitFrames;
        const uint32_t nf = (uint32_t)((p.n - f0) < kStUnitFrames ? (p.n - f0) : kStUnitFrames);
        // ---- take the unit only if its frames are packed and 64..1536 B ----
        uint64_t S[kQ];
        uint32_t Ln[kQ];
        const bool bad = unit_unpacked(p, f0, nf, lane, S, Ln);
        if (__any(bad)) {
            if (!LOAD && lane == 0) p.ulist[atomicAdd(p.ucount, 1u)] = (uint32_t)u;
            continue;
        }
        // ---- geometry, relative to X0 (the first item's start) ----
        const uint64_t s0 = p.base + (((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(S[0] >> 32)) << 32) |
                                      (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)S[0]));
#ifdef FCS_ST_ALIGN16
        const uint64_t X0 = s0 & ~15ull;
#else
        const uint64_t lo16 = p.lo4 & ~15ull;
        const uint64_t X0 = (s0 & ~127ull) > lo16 ? (s0 & ~127ull) : lo16;
#endif
        dma_item(X0);
        const uint64_t o0 = X0 - p.base;   // arena offset of X0
        const uint32_t last = nf - 1;
        // every frame of the unit: end (relative to X0) << 11 | length
        uint32_t pk[kQ];
#pragma unroll
        for (int q = 0; q < kQ; q++) pk[q] = ((uint32_t)(S[q] + Ln[q] - o0) << kStLenBits) | Ln[q];
        uint32_t E = 0;   // the unit's end
#pragma unroll
        for (int q = 0; q < kQ; q++)
            if ((last >> 6) == (uint32_t)q) E = (uint32_t)__builtin_amdgcn_readlane((int)pk[q], (int)(last & 63u)) >> kStLenBits;
        // The cursor: frames 64 cb + lane (batch A, pk[0]) and 64 (cb + 1) + lane (batch B, pk[1]);
        // the batches after them follow in pk[2..] (shifted down as the cursor moves: no indexed
        // register access, which the compiler would turn into scratch memory). An item's starts lie
        // in batches A and B (frames >= 64 B).
        uint32_t cb = 0;
        const uint32_t nitems = (E + kStItem - 1) / kStItem;
#ifdef FCS_STAMPS
        {
            ST_T(tu1)
            sts[0] += tu1 - tu0;
            sts[6]++;
        }
#endif
        uint32_t nsf = 0, base_cnt = 0, closed = 0;
        uint32_t tend = 0;   // end tap of the unit's last frame (0 when it ends on an item edge)
        // close frames 64 b .. 64 b + cnt - 1 (all ended; pw: their end << 11 | length): start term,
        // end tap, one 256-B store
        auto close_pass = [&](uint32_t b, uint32_t cnt, uint32_t pw) {
            wave_lds_sync();
            const uint32_t g = 64u * b + (uint32_t)lane;
            const uint32_t e = pw >> kStLenBits, L = pw & kLenMask;
            const uint32_t st = e - L, ss = st & 63u, se = e & 63u;
            const uint32_t Ts = tap[g & 127u];
            const uint32_t Te = g < last ? tap[(g + 1u) & 127u] : tend;
            const uint32_t a0 = acc[g & 127u];
            wave_lds_sync();
            acc[g & 127u] = 0u;
#ifdef FCS_ST_ABL_NOCLOSE   // measurement-only: the close's four shifts replaced by XORs (wrong FCS)
            const uint32_t reg = Ts ^ Te ^ a0 ^ k1_of(ss) ^ se;
#else
            const uint32_t U = hole_shift(lds, Ts, kStHoleWord + 4u * (15u - (ss >> 2)), k1_of(ss));
            const uint32_t js = (uint32_t)lane < cnt ? (e >> 6) - (st >> 6) - 1u : 0u;
            const uint32_t a = hole_shift(lds, U, kStHoleChunk + 4u * js, a0);
            const uint32_t inner = hole_shift(lds, a, kStHoleWord + 4u * ((se >> 2) + 1u), Te);
            const uint32_t reg = hole_shift(lds, inner, kStHoleInv + 4u * (3u - (se & 3u)), 0u);
#endif
            emit<kStBad>(p, lds, (uint32_t)lane < cnt, f0 + g, ~reg);
        };
        if (LOAD) {   // the item walk alone: slot wait, word reads, next DMA
            for (uint32_t t = 0; t < nitems; t++) {
                const uint32_t Xr = kStItem * t;
                __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0)
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const u32x4 x = *pc[i];
                    lx ^= x.x ^ x.y ^ x.z ^ x.w;
                }
                __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
                if (t + 1 < nitems) dma_item(X0 + Xr + kStItem);
            }
            wave_lds_sync();
            continue;
        }
        for (uint32_t t = 0; t < nitems; t++) {
            const uint32_t Xr = kStItem * t;
            ST_T(ti0)
            // ---- marks: frames starting in this item, and the unit's end ----
            const uint32_t gA = 64u * cb + (uint32_t)lane, gB = gA + 64u;
            const uint32_t eA = pk[0] >> kStLenBits, eB = pk[1] >> kStLenBits;
            const uint32_t sA = eA - (pk[0] & kLenMask), sB = eB - (pk[1] & kLenMask);
            const bool inA = gA >= nsf && gA < nf && sA < Xr + kStItem;
            const bool inB = gB >= nsf && gB < nf && sB < Xr + kStItem;
            if (inA) *mark_at((sA - Xr) >> 6) = kMarkStart | (gA << 6) | ((sA - Xr) & 63u);
            if (inB) *mark_at((sB - Xr) >> 6) = kMarkStart | (gB << 6) | ((sB - Xr) & 63u);
            if (E < Xr + kStItem && lane == 0) *mark_at((E - Xr) >> 6) = kMarkEnd | ((E - Xr) & 63u);
            nsf += (uint32_t)__popcll(__ballot(inA)) + (uint32_t)__popcll(__ballot(inB));
            // chunk of the next boundary past this item: the end of the last frame started so far
            const uint32_t gl = nsf - 1u;
            const uint32_t el = (uint32_t)__builtin_amdgcn_readlane((int)((gl >> 6) == cb ? eA : eB), (int)(gl & 63u));
            const uint32_t le_far = (el - Xr) >> 6;
            wave_lds_sync();
            const uint32_t mk = lds_rd(lds, mark_lane);
            *reinterpret_cast<uint32_t *>(lds + mark_lane) = 0u;
            const bool isst = (mk & kMarkStart) != 0, isend = (mk & kMarkEnd) != 0;
            const uint32_t sig = mk & 63u, k = sig >> 2, r = sig & 3u, bf = (mk >> 6) & 1023u;
            const uint64_t Mst = __ballot(isst), Mend = __ballot(isend), Mb = Mst | Mend;
            const uint64_t upto = Mst & ((2ull << lane) - 1ull);                // starts at or before this lane
            const int o = (int)(base_cnt + (uint32_t)__popcll(upto)) - 1;     // frame holding the chunk's last byte
            const bool contrib = o >= 0 && Xr + 64u * (uint32_t)lane + 63u < E;
            const uint64_t after = lane == 63 ? 0ull : (Mb & (~0ull << (lane + 1)));
            const uint32_t le = after ? (uint32_t)__builtin_ctzll(after) : le_far;
            const uint32_t j = contrib ? le - (uint32_t)lane - 1u : 0u;

            // ---- this item's bytes; the next item's DMA ----
            ST_T(ti1)
            __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's item has landed
            ST_T(ti2)
#ifdef FCS_STAMPS
            sts[1] += ti1 - ti0;
            sts[2] += ti2 - ti1;
#endif
            uint32_t w[16];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const u32x4 x = *pc[i];
                w[4 * i] = x.x;
                w[4 * i + 1] = x.y;
                w[4 * i + 2] = x.z;
                w[4 * i + 3] = x.w;
            }
            // the tap word: word k & 3 of piece k / 4
            const uint32_t wk = lds_rd(slot, cbase + 16u * (((k >> 2) + sw) & 3u) + 4u * (k & 3u));
            __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA
            if (t + 1 < nitems) dma_item(X0 + Xr + kStItem);

            // ---- the chain over 16 words; its state before word k ----
            uint32_t x = w[0], xk = 0;
#ifdef FCS_ST_NOCRC   // measurement-only: the words XORed instead of the chain (wrong FCS)
#pragma unroll
            for (int i = 1; i < 16; i++) x ^= w[i];
            xk = x ^ k;
#elif FCS_ST_CHAINS == 2
            // two independent 8-word chains, c0 over words 0..7 and c1 over 8..15, each from register
            // 0 (half the dependent lookups of one chain): L = A_32(c0) ^ c1, and the state before
            // word k >= 8 is c1_{k-8} ^ A_{4 (k-8)}(c0), so that tap adds A_{4 (k-7)}(c0)
            uint32_t y = w[8];
#pragma unroll
            for (int i = 0; i < 8; i++) {
                if ((uint32_t)i == k) xk = x;
                if ((uint32_t)(i + 8) == k) xk = y;
                x = step4_l8(lds, x, i < 7 ? w[i + 1] : 0u, B, SEL);
                y = step4_l8(lds, y, i < 7 ? w[i + 9] : 0u, B, SEL);
            }
            const uint32_t c0 = x;
            x = hole_shift(lds, c0, kStHoleWord + 4u * 8u, y);
#else
#pragma unroll
            for (int i = 0; i < 16; i++) {
                if ((uint32_t)i == k) xk = x;
                x = step4_l8(lds, x, i < 15 ? w[i + 1] : 0u, B, SEL);
            }
#endif
            // the tap: word k's bytes before the boundary finish the prefix (x_k ^ w_k = s_k)
#if FCS_ST_CHAINS == 2 && !defined(FCS_ST_NOCRC)
            const uint32_t Tp = hole_shift(lds, k >= 8u ? c0 : 0u, kStHoleWord + 4u * (k >= 8u ? k - 7u : 0u),
                                           step4_l8(lds, xk ^ (wk & (0xFFFFFFFFu << (8u * r))), 0u, B, SEL));
#else
            const uint32_t Tp = step4_l8(lds, xk ^ (wk & (0xFFFFFFFFu << (8u * r))), 0u, B, SEL);
#endif
            if (isst) tap[bf & 127u] = Tp;
            if (Mend) tend = (uint32_t)__builtin_amdgcn_readlane((int)Tp, (int)__builtin_ctzll(Mend));
#ifdef FCS_STAMPS
            ST_T(ti3)
            sts[3] += ti3 - ti2;
#endif

            // ---- chunk contributions: the lane ending a frame's run of lanes adds the run's sum ----
#ifdef FCS_ST_ABL_NOSHIFT   // measurement-only: no chunk shift (wrong FCS)
            const uint32_t Wc = x ^ j;
#elif defined(FCS_ST_SKIPJ0)   // measurement-only: lanes with j = 0 (A_0 = identity) skip the lookups
            uint32_t Wc = x;
            if (j) Wc = hole_shift(lds, x, kStHoleChunk + 4u * j, 0u);
#else
            const uint32_t Wc = hole_shift(lds, x, kStHoleChunk + 4u * j, 0u);
#endif
#ifdef FCS_ST_PROBE_LDS   // measurement-only: N extra conflict-free LDS reads per item, off the critical path
#pragma unroll
            for (int i = 0; i < FCS_ST_PROBE_LDS; i++) probe ^= lds_rd(lds, ((uint32_t)lane & 31u) * 4u + (uint32_t)i * 256u);
#endif
#ifdef FCS_ST_PROBE_VALU   // measurement-only: N extra VALU operations per item, off the critical path
#pragma unroll
            for (int i = 0; i < FCS_ST_PROBE_VALU; i++) probe = xor3(probe, w[i & 15], (uint32_t)i) + (uint32_t)i;
#endif
            const uint32_t P = wave_xor_scan(contrib ? Wc : 0u);
            // the run of this lane's frame starts at the last start at or before it (if any); its sum
            // is P here minus P just before that start
            const int sl = upto ? 63 - __builtin_clzll(upto) : 0;
            const uint32_t Pb = (uint32_t)__shfl((int)P, sl > 0 ? sl - 1 : 0);
            const bool seg_end = lane == 63 || ((Mst >> (lane + 1)) & 1ull);
            const uint32_t v = P ^ (sl > 0 ? Pb : 0u);
            if (o >= 0 && seg_end && v) {
                uint32_t *ap = &acc[(uint32_t)o & 127u];
                *ap = *ap ^ v;
            }
            base_cnt += (uint32_t)__popcll(Mst);
            // frames before the last one starting here have ended (all of them at the unit's end);
            // a cursor batch all of whose frames have ended closes, and the cursor moves on
            uint32_t ended = closed;
            if (Mst) ended = (uint32_t)__builtin_amdgcn_readlane((int)bf, 63 - __builtin_clzll(Mst));
            if (Mend) ended = nf;
            if (ended >= 64u * (cb + 1u) && 64u * (cb + 1u) <= last) {
                close_pass(cb, 64u, pk[0]);
                closed = 64u * (cb + 1u);
                cb++;
#pragma unroll
                for (int q = 0; q + 1 < kQ; q++) pk[q] = pk[q + 1];
            }
#ifdef FCS_STAMPS
            ST_T(ti4)
            sts[4] += ti4 - ti3;
            sts[5]++;
#endif
        }
        // the last batch (A, or B when A closed in the last item) closes at the unit's end
        if (closed < nf) {
            if ((closed >> 6) == cb) close_pass(cb, nf - closed, pk[0]);
            else close_pass(cb + 1u, nf - closed, pk[1]);
            closed = nf;
        }
        wave_lds_sync();
    }
#ifdef FCS_STAMPS
    if (p.dbg != nullptr && lane == 0) {
        sts[7] = __builtin_amdgcn_s_memtime() - st_begin;
        const uint32_t wv = blockIdx.x * kStWaves + wave;
#pragma unroll
        for (int i = 0; i < 8; i++) p.dbg[wv * 8 + i] = sts[i];
    }
#endif
    if (LOAD) {   // keep the word reads live: a store no realistic input triggers
        if (lx == 0x5EEDF00Du && p.out) p.out[0] = lx;
        return;
    }
#if defined(FCS_ST_PROBE_LDS) || defined(FCS_ST_PROBE_VALU)
    if (probe == 0x5EEDF00Du && p.out) p.out[0] = probe;
#endif
    flush_bad<kStBad>(p, lds);
}

// Counter-based byte generator: 8-byte word q of the stream = splitmix64(seed + q).
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ __launch_bounds__(256) void fill_splitmix_kernel(uint8_t *p, uint64_t bytes,
                                                            uint64_t seed, uint64_t off) {
    const uint64_t tid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t nth = (uint64_t)gridDim.x * blockDim.x;
    const uint64_t head = (8 - (off & 7)) & 7;   // bytes before the first aligned stream word
    for (uint64_t i = tid; i < head && i < bytes; i += nth) {
        const uint64_t q = off + i;
        p[i] = (uint8_t)(splitmix64(seed + (q >> 3)) >> (8 * (q & 7)));
    }
    if (bytes <= head) return;
    const uint64_t body_words = (bytes - head) / 8;
    const uint64_t w0 = (off + head) >> 3;
    uint8_t *pb = p + head;
    const bool al8 = (((uintptr_t)pb) & 7) == 0;
    for (uint64_t i = tid; i < body_words; i += nth) {
        const uint64_t v = splitmix64(seed + w0 + i);
        if (al8) {
            reinterpret_cast<uint64_t *>(pb)[i] = v;
        } else {
#pragma unroll
            for (int b = 0; b < 8; b++) pb[8 * i + b] = (uint8_t)(v >> (8 * b));
        }
    }
    for (uint64_t i = head + body_words * 8 + tid; i < bytes; i += nth) {
        const uint64_t q = off + i;
        p[i] = (uint8_t)(splitmix64(seed + (q >> 3)) >> (8 * (q & 7)));
    }
}

// Pure read stream: 16 B per lane per load, 4 loads in flight, XOR folded to one word per thread.
__global__ __launch_bounds__(256) void read_stream_kernel(const u32x4 *__restrict__ p, uint64_t n16,
                                                          uint32_t *sink) {
    uint32_t acc = 0;
    const uint64_t st = (uint64_t)gridDim.x * blockDim.x;
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t pb = (uint64_t)p;
    for (; i + 3 * st < n16; i += 4 * st) {
        const u32x4 a = gload<u32x4>(pb + 16 * i), b = gload<u32x4>(pb + 16 * (i + st)),
                    c = gload<u32x4>(pb + 16 * (i + 2 * st)), e = gload<u32x4>(pb + 16 * (i + 3 * st));
        acc ^= a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w ^ c.x ^ c.y ^ c.z ^ c.w ^ e.x ^ e.y ^
               e.z ^ e.w;
    }
    for (; i < n16; i += st) {
        const u32x4 a = p[i];
        acc ^= a.x ^ a.y ^ a.z ^ a.w;
    }
    if (acc == 0x9E3779B9u) sink[0] = acc;   // keep the loads live; practically never stores
}

// Completion signal for small host batches: launched behind the FCS kernel on the same stream,
// it stores `v` into a device-mapped host word, on which the host spins instead of synchronising
// the stream (cuts the hipStreamSynchronize wake-up from the round trip).
// Test-only (the fault-hook build's fcs_debug_hold_small): one lane waits until the host stores a
// nonzero value into the mapped word, or until `ticks` of the 100 MHz constant clock have passed, so
// every wave reaches its exit. System-scope atomic loads: vector loads that bypass the caches.
__global__ void hold_kernel(const uint32_t *word, uint64_t ticks) {
    if (threadIdx.x != 0) return;
    const uint64_t t0 = wall_clock64();
    while (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) == 0u &&
           wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(64);
}

__global__ void signal_kernel(uint64_t *flag, uint64_t v) {
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
        __hip_atomic_store(flag, v, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The single-frame tables (7 KiB) into LDS: every load issued before the first store, so the
// wave waits for one memory latency instead of seven in a row.
__device__ __forceinline__ void stage_one_blob(uint32_t *t, const uint32_t *blob, int lane) {
    constexpr int kIters = kOneBlobWords / 4 / 64;
    static_assert(kOneBlobWords % 256 == 0, "one 16-byte piece per lane per step");
    u32x4a4 v[kIters];
#pragma unroll
    for (int k = 0; k < kIters; k++) v[k] = reinterpret_cast<const u32x4a4 *>(blob)[lane + 64 * k];
#pragma unroll
    for (int k = 0; k < kIters; k++) reinterpret_cast<u32x4a4 *>(t)[lane + 64 * k] = v[k];
}

// Drop-in ether_fcs for one frame (fcs_launch.hpp OneArgs). The frame arrives in the kernel
// arguments, right-aligned in a 1536-byte window with zeros in front: from a zero register,
// leading zeros change nothing, and the all-ones start of the real CRC is added back as
// kinit = A_len(0xFFFFFFFF) (the register update is affine: R(s, M) = A_len(s) ^ R(0, M)).
// Lane j runs six slice-by-4 steps over window bytes [24j, 24j + 24) from a zero register; a
// six-level tree then joins neighbouring lane groups, the earlier one advanced by A_{24 * 2^k}.
// Lane 0 stores (seq << 32) | FCS into a mapped host word with one system-scope store, which
// is also the completion signal the host spins on: no staging copy, no second launch.
__device__ __forceinline__ uint32_t one_step(const uint32_t *t, uint32_t x, uint32_t wn) {
    return xor3(xor3(t[768 + (x & 0xFFu)], t[512 + ((x >> 8) & 0xFFu)], t[256 + ((x >> 16) & 0xFFu)]),
                t[x >> 24], wn);
}

__global__ __launch_bounds__(64) void fcs_one_kernel(OneArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t t[kOneBlobWords];
    const int lane = threadIdx.x;
#ifndef FCS_ONE_NOBLOB   // measurement-only build: tables not staged (wrong FCS; timing only)
    stage_one_blob(t, a.blob, lane);
#endif
    // the window words straight from the kernel-argument segment (no private copy of `a`)
    typedef const __attribute__((address_space(4))) uint32_t karg_u32;
    karg_u32 *dw = reinterpret_cast<karg_u32 *>(
        (const __attribute__((address_space(4))) uint8_t *)__builtin_amdgcn_kernarg_segment_ptr() +
        offsetof(OneArgs, data));
    uint32_t w[6];
#ifdef FCS_ONE_NOARG   // measurement-only build: the frame words not read (wrong FCS; timing only)
#pragma unroll
    for (int q = 0; q < 6; q++) w[q] = lane * 6 + q;
    (void)dw;
#else
#pragma unroll
    for (int q = 0; q < 6; q++) w[q] = dw[lane * 6 + q];
#endif
    __syncthreads();
    uint32_t x = w[0];
#pragma unroll
    for (int i = 0; i < 6; i++) x = one_step(t, x, i < 5 ? w[i + 1] : 0u);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint32_t *nt = t + 1024 + k * 128;
        uint32_t y = x;
        if (!(lane & (1 << k))) {   // the earlier group: advance it past the later one's bytes
            uint32_t r[8];
#pragma unroll
            for (int q = 0; q < 8; q++) r[q] = nt[q * 16 + ((x >> (4 * q)) & 15u)];
            y = xor9(r, 0u);
        }
        x = y ^ (uint32_t)__shfl_xor((int)y, 1 << k);
    }
    if (lane == 0)
        __hip_atomic_store(a.flag, ((uint64_t)a.seq << 32) | (uint64_t)(uint32_t)~(x ^ a.kinit), __ATOMIC_RELEASE,
                           __HIP_MEMORY_SCOPE_SYSTEM);
}

// One wave's frame of at most kOneBytes bytes ending at `end` and starting at `start`, read from
// (mapped) memory: the same window, lane chain and tree as fcs_one_kernel. The wave first copies
// the 16-byte blocks that hold the frame into its LDS window with coalesced 16-byte loads (host
// memory over PCIe wants few, wide requests), then every lane takes its 24 bytes from there.
// Blocks start with the one holding `start` and end with the one holding end - 1: no byte of
// another page is touched (the frame may open or close its allocation). The realignment's last
// LDS dword may reach past the copied bytes; those bytes lie beyond the lane's 24 and are unused.
constexpr uint32_t kOneWinBytes = kOneBytes + 32;   // per-wave LDS window (16-B aligned base)

// The tables (blob, staged into t) and the frame are fetched together: every load of both is
// issued before the first LDS store, so the table latency hides under the frame's PCIe reads.
__device__ __forceinline__ uint32_t one_frame_reg(uint32_t *t, const uint32_t *blob, uint8_t *win, uint64_t start,
                                                  uint64_t end, int lane) {
    const uint64_t wbase = end - kOneBytes;            // window byte 0 (may precede the frame)
    const uint64_t g0 = wbase & ~15ull;                // LDS byte 0 <-> this address
    const uint64_t b0 = (start > wbase ? start : wbase) & ~15ull;
    const uint64_t b1 = (end + 15) & ~15ull;           // one past the last block to load
    constexpr int kTab = kOneBlobWords / 4 / 64;
    constexpr int kBlk = (kOneWinBytes / 16 + 63) / 64;
    u32x4a4 tv[kTab], fv[kBlk];
#pragma unroll
    for (int k = 0; k < kTab; k++) tv[k] = reinterpret_cast<const u32x4a4 *>(blob)[lane + 64 * k];
#pragma unroll
    for (int k = 0; k < kBlk; k++) {
        const uint64_t a = b0 + 16 * (uint64_t)(lane + 64 * k);
        if (a < b1) fv[k] = gload<u32x4a4>(a);
    }
#pragma unroll
    for (int k = 0; k < kTab; k++) reinterpret_cast<u32x4a4 *>(t)[lane + 64 * k] = tv[k];
#pragma unroll
    for (int k = 0; k < kBlk; k++) {
        const uint64_t a = b0 + 16 * (uint64_t)(lane + 64 * k);
        if (a < b1) *reinterpret_cast<u32x4a4 *>(win + (a - g0)) = fv[k];
    }
    __syncthreads();
    const int64_t c = (int64_t)wbase + 24 * lane;      // this lane's window bytes [c, c + 24)
    uint32_t w[6] = {0, 0, 0, 0, 0, 0};
    if (c + 24 > (int64_t)start) {
        const uint32_t p = (uint32_t)((uint64_t)c - g0);
        const uint32_t r = p & 3u;
        uint32_t d[7];
#pragma unroll
        for (int q = 0; q < 7; q++) d[q] = *reinterpret_cast<const uint32_t *>(win + (p & ~3u) + 4 * q);
        const int zr = (int)((int64_t)start - c);      // window bytes before the frame: masked
#pragma unroll
        for (int i = 0; i < 6; i++) {
            const uint32_t v = __builtin_amdgcn_alignbyte(d[i + 1], d[i], r);
            int z = zr - 4 * i;
            z = z < 0 ? 0 : (z > 4 ? 4 : z);
            w[i] = v & (uint32_t)(0xFFFFFFFFull << (8 * z));
        }
    }
    wave_lds_sync();                                   // window reads done before the next frame's copy
    uint32_t x = w[0];
#pragma unroll
    for (int i = 0; i < 6; i++) x = one_step(t, x, i < 5 ? w[i + 1] : 0u);
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const uint32_t *nt = t + 1024 + k * 128;
        uint32_t y = x;
        if (!(lane & (1 << k))) {
            uint32_t r8[8];
#pragma unroll
            for (int q = 0; q < 8; q++) r8[q] = nt[q * 16 + ((x >> (4 * q)) & 15u)];
            y = xor9(r8, 0u);
        }
        x = y ^ (uint32_t)__shfl_xor((int)y, 1 << k);
    }
    return x;
}

// A small-batch frame's result: RX verify writes ok[f] (the frame carries its trailer; it checks
// iff the residue shows), TX writes out[f] (the host stores it little-endian right after the frame,
// src/linux/ether.c:263, once the batch is complete). Both arrays are the library's own mapped
// memory. Then the frame counts itself done; the batch's last frame stores seq.
__device__ __forceinline__ void small_finish(uint32_t fcs, uint8_t *ok, uint32_t *out, uint32_t f, uint32_t L,
                                             int lane, unsigned long long *count, uint64_t count_base, uint32_t n,
                                             uint64_t *flag, uint64_t seq) {
    if (lane == 0) {
        if (ok) ok[f] = (L >= 4 && fcs == 0x2144DF1Cu) ? 1 : 0;
        else out[f] = fcs;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");   // this frame's result has reached host memory
    if (lane == 0) {
        const uint64_t done = __hip_atomic_fetch_add(count, 1ull, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        if (done == count_base + n - 1)   // the batch's last frame
            __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// One workgroup (one wave) per frame, so the frames' PCIe reads come from as many CUs: one CU
// reading 16 frames of host memory took 17.7 us, against 10.6 us for one. Each wave writes its
// FCS (or check), makes it visible system-wide and counts itself done on a device counter; the
// last one to finish stores `seq` into the mapped completion word.
__global__ __launch_bounds__(64) void fcs_tx_small_kernel(TxSmallArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t t[kOneBlobWords];
    __shared__ __attribute__((aligned(16))) uint8_t win[kOneWinBytes];
    const int lane = threadIdx.x;
    const uint32_t f = blockIdx.x;
    typedef const __attribute__((address_space(4))) uint8_t karg_u8;
    karg_u8 *ka = (karg_u8 *)__builtin_amdgcn_kernarg_segment_ptr();
    const uint64_t o = *(const __attribute__((address_space(4))) uint64_t *)(ka + offsetof(TxSmallArgs, off) + 8 * f);
    const uint32_t L = *(const __attribute__((address_space(4))) uint32_t *)(ka + offsetof(TxSmallArgs, len) + 4 * f);
    const uint32_t ki = *(const __attribute__((address_space(4))) uint32_t *)(ka + offsetof(TxSmallArgs, kinit) + 4 * f);
    const uint64_t start = (uint64_t)a.base + o;
    const uint32_t x = one_frame_reg(t, a.blob, win, start, start + L, lane);
    small_finish(~(x ^ ki), a.ok, a.out, f, L, lane, a.count, a.count_base, a.n, a.flag, a.seq);
}

__global__ __launch_bounds__(64) void fcs_small_list_kernel(ListArgs a) {
    __shared__ __attribute__((aligned(16))) uint32_t t[kOneBlobWords];
    __shared__ __attribute__((aligned(16))) uint8_t win[kOneWinBytes];
    const int lane = threadIdx.x;
    const uint32_t f = blockIdx.x;
    const uint64_t o = a.off[f];      // one mapped read each (uniform address)
    const uint32_t L = a.len[f];
    const uint32_t ki = a.kinit[L < kOneBytes ? L : kOneBytes];
    const uint64_t start = (uint64_t)a.base + o;
    const uint32_t x = one_frame_reg(t, a.blob, win, start, start + L, lane);
    small_finish(~(x ^ ki), a.ok, a.out, f, L, lane, a.count, a.count_base, a.n, a.flag, a.seq);
}

// TX mode helper: after the FCS kernel wrote crc[i], store it little-endian after each frame.
__global__ __launch_bounds__(256) void tx_store_kernel(uint8_t *base, uint64_t stride,
                                                       const uint32_t *len, const uint32_t *crc,
                                                       uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint8_t *q = base + i * stride + len[i];
    const uint32_t c = crc[i];
    q[0] = (uint8_t)c;
    q[1] = (uint8_t)(c >> 8);
    q[2] = (uint8_t)(c >> 16);
    q[3] = (uint8_t)(c >> 24);
}

// ---- host-side launchers (the engine TU never names the kernels) ----
// Variable-length batches (and nothing else): windowed = throughput form (64-frame windows per wave,
// chunks dealt flat to the lanes), otherwise one quarter-wave per frame, every frame in flight at
// once (small batches).
hipError_t launch_fcs(bool var, bool windowed, const KParams &p, int grid, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (!var) return hipErrorInvalidValue;   // fixed-length batches: launch_fixed_route
    const bool tiny = fixed_tiny(p);
    if (!windowed) {
        if (tiny) hipLaunchKernelGGL((fcs_kernel<true, true, false, kWgThreads>), dim3(grid), dim3(kWgThreads), 0, st, p);
        else hipLaunchKernelGGL((fcs_kernel<true, false, false, kWgThreads>), dim3(grid), dim3(kWgThreads), 0, st, p);
    } else if (tiny) {
        hipLaunchKernelGGL((fcs_flat_kernel<true>), dim3(grid), dim3(kWgThreads), 0, st, p);
    } else {
        hipLaunchKernelGGL((fcs_flat_kernel<false>), dim3(grid), dim3(kWgThreads), 0, st, p);
    }
    return hipGetLastError();
}

namespace {
std::atomic<uint64_t> g_last_fixed{0};   // the last launch_fixed_route launch, packed (kernel, wd, threads)
}

FixedRoute last_fixed_launch() {
    const uint64_t v = g_last_fixed.load(std::memory_order_relaxed);
    FixedRoute r{};
    r.kernel = (FixedKernel)(v & 0xFF);
    r.wd = (int)((v >> 8) & 0xFFFF);
    r.threads = (int)((v >> 24) & 0xFFFF);
    r.tiny = (v >> 40) & 1;
    return r;
}

// Launches exactly the kernel route_fixed named: each case records what it launched (kernel, its
// window or mask template argument, workgroup size), so a test can compare the launch with the
// route (tests/test_gpu_routing.py).
hipError_t launch_fixed_route(const FixedRoute &r, const KParams &p, int grid, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    auto rec = [](FixedKernel k, int wd, int threads, bool tiny) {
        g_last_fixed.store((uint64_t)k | ((uint64_t)(uint16_t)wd << 8) | ((uint64_t)(uint16_t)threads << 24) |
                               ((uint64_t)tiny << 40),
                           std::memory_order_relaxed);
    };
#define FCS_GO(K, WD, T, TINY, ...)                                             \
    do {                                                                        \
        hipLaunchKernelGGL(__VA_ARGS__, dim3(grid), dim3(T), 0, st, p);         \
        rec(K, WD, T, TINY);                                                    \
    } while (0)
    switch (r.kernel) {
    case FixedKernel::kShort:
        switch (r.wd) {
            case 16: FCS_GO(FixedKernel::kShort, 16, kWgThreads, false, fcs_short_kernel<16>); break;
            case 24: FCS_GO(FixedKernel::kShort, 24, kWgThreads, false, fcs_short_kernel<24>); break;
            case 32: FCS_GO(FixedKernel::kShort, 32, kWgThreads, false, fcs_short_kernel<32>); break;
            default: return hipErrorInvalidValue;
        }
        break;
    case FixedKernel::kFlat:
        if (r.tiny) FCS_GO(FixedKernel::kFlat, 0, kWgThreads, true, fcs_flat_kernel<true>);
        else FCS_GO(FixedKernel::kFlat, 0, kWgThreads, false, fcs_flat_kernel<false>);
        break;
    case FixedKernel::kWide4:
#define FCS_WIDE4(W) \
    case W: FCS_GO(FixedKernel::kWide4, W, wide_threads(W), false, (fcs_wide_kernel<W, 4>)); break;
        switch (r.wd) {
            FCS_WIDE4(9) FCS_WIDE4(10) FCS_WIDE4(11) FCS_WIDE4(12) FCS_WIDE4(13) FCS_WIDE4(14) FCS_WIDE4(15)
            FCS_WIDE4(16) FCS_WIDE4(18) FCS_WIDE4(19) FCS_WIDE4(20) FCS_WIDE4(21) FCS_WIDE4(22) FCS_WIDE4(23)
            FCS_WIDE4(24) FCS_WIDE4(25) FCS_WIDE4(26)
            default: return hipErrorInvalidValue;
        }
#undef FCS_WIDE4
        break;
    case FixedKernel::kWide8:
#define FCS_WIDE8(W) \
    case W: FCS_GO(FixedKernel::kWide8, W, wide_threads(W), false, (fcs_wide_kernel<W, 8>)); break;
        switch (r.wd) {
            FCS_WIDE8(11) FCS_WIDE8(12) FCS_WIDE8(14) FCS_WIDE8(15) FCS_WIDE8(16) FCS_WIDE8(18) FCS_WIDE8(19)
            FCS_WIDE8(20) FCS_WIDE8(22) FCS_WIDE8(23) FCS_WIDE8(24) FCS_WIDE8(26) FCS_WIDE8(27) FCS_WIDE8(28)
            default: return hipErrorInvalidValue;
        }
#undef FCS_WIDE8
        break;
    case FixedKernel::kWide16:
#define FCS_WIDE(W) \
    case W: FCS_GO(FixedKernel::kWide16, W, wide_threads(W), false, fcs_wide_kernel<W>); break;
        switch (r.wd) {
#if FCS_WIDE_MID_WD_MIN <= 11   // the mid-length widths from kWideMidMin (11 .. 12: measurement builds)
            FCS_WIDE(11)
#endif
#if FCS_WIDE_MID_WD_MIN <= 12
            FCS_WIDE(12)
#endif
#if FCS_WIDE_MID_WD_MIN <= 14
            FCS_WIDE(14)
#endif
#if FCS_WIDE_MID_WD_MIN <= 15
            FCS_WIDE(15)
#endif
#if FCS_WIDE_MID_WD_MIN <= 16
            FCS_WIDE(16)
#endif
#if FCS_WIDE_MID_WD_MIN <= 18
            FCS_WIDE(18)
#endif
#if FCS_WIDE_MID_WD_MIN <= 19
            FCS_WIDE(19)
#endif
            FCS_WIDE(20) FCS_WIDE(22) FCS_WIDE(23) FCS_WIDE(24) FCS_WIDE(26) FCS_WIDE(30) FCS_WIDE(32)
            default: return hipErrorInvalidValue;
        }
#undef FCS_WIDE
        break;
    case FixedKernel::kSegment:
        switch (r.wd) {
            case 24: FCS_GO(FixedKernel::kSegment, 24, kSegilThreads, false, fcs_segil_kernel); break;
#define FCS_SEGW(W) \
    case W: FCS_GO(FixedKernel::kSegment, W, kSegilThreads, false, fcs_segw_kernel<W>); break;
            FCS_SEGW(15) FCS_SEGW(16) FCS_SEGW(18) FCS_SEGW(19) FCS_SEGW(20) FCS_SEGW(22) FCS_SEGW(23)
            FCS_SEGW(26) FCS_SEGW(30) FCS_SEGW(32)
#undef FCS_SEGW
            default: return hipErrorInvalidValue;
        }
        break;
    case FixedKernel::kDma:
        if (r.wd == 2) FCS_GO(FixedKernel::kDma, 2, kDmaWgThreads, false, (fcs_dma_kernel<2, false>));
        else if (r.wd == kSingleMaskWords) FCS_GO(FixedKernel::kDma, kSingleMaskWords, kDmaWgThreads, false, (fcs_dma_kernel<kSingleMaskWords, false>));
        else return hipErrorInvalidValue;
        break;
    case FixedKernel::kTiny:
        if (r.wd) FCS_GO(FixedKernel::kTiny, 1, kWgThreads, true, (fcs_kernel<false, true, true, kWgThreads>));
        else FCS_GO(FixedKernel::kTiny, 0, kWgThreads, true, (fcs_kernel<false, true, false, kWgThreads>));
        break;
    case FixedKernel::kSingle:
#ifdef FCS_OLD_SINGLE   // measurement-only build: generic kernel's SINGLE instantiation
        FCS_GO(FixedKernel::kSingle, 0, kWgThreads, false, (fcs_kernel<false, false, true, kWgThreads>));
#else
        FCS_GO(FixedKernel::kSingle, 0, kFixedWgThreads, false, fcs_single_kernel);
#endif
        break;
    case FixedKernel::kGeneric:
        if (r.threads == kFixedWgThreads)
            FCS_GO(FixedKernel::kGeneric, 0, kFixedWgThreads, false, (fcs_kernel<false, false, false, kFixedWgThreads>));
        else
            FCS_GO(FixedKernel::kGeneric, 0, kWgThreads, false, (fcs_kernel<false, false, false, kWgThreads>));
        break;
    }
#undef FCS_GO
    return hipGetLastError();
}

hipError_t launch_hold(const uint32_t *word, uint64_t ticks, hipStream_t st) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(hold_kernel, dim3(1), dim3(64), 0, st, word, ticks);
    return hipGetLastError();
}

hipError_t launch_signal(uint64_t *flag, uint64_t v, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(64), 0, st, flag, v);
    return hipGetLastError();
}

hipError_t launch_fill(void *p, uint64_t bytes, uint64_t seed, uint64_t off, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    uint64_t words = bytes / 8 + 1;
    int grid = (int)((words + 255) / 256);
    if (grid > 8192) grid = 8192;
    if (grid < 1) grid = 1;
    hipLaunchKernelGGL(fill_splitmix_kernel, dim3(grid), dim3(256), 0, st, (uint8_t *)p, bytes, seed, off);
    return hipGetLastError();
}

hipError_t launch_read_stream(const void *p, uint64_t bytes, uint32_t *sink, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    hipLaunchKernelGGL(read_stream_kernel, dim3(8192), dim3(256), 0, st, (const u32x4 *)p, bytes / 16, sink);
    return hipGetLastError();
}

hipError_t launch_dma_stream(const KParams &p, int grid, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    hipLaunchKernelGGL((fcs_dma_kernel<2, true>), dim3(grid), dim3(kDmaWgThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_short(const KParams &p, int grid, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    switch (short_wd(p.flen)) {
        case 16: hipLaunchKernelGGL(fcs_short_kernel<16>, dim3(grid), dim3(kWgThreads), 0, st, p); break;
        case 24: hipLaunchKernelGGL(fcs_short_kernel<24>, dim3(grid), dim3(kWgThreads), 0, st, p); break;
        case 32: hipLaunchKernelGGL(fcs_short_kernel<32>, dim3(grid), dim3(kWgThreads), 0, st, p); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_stream(const KParams &p, int grid, hipStream_t st, bool load_only) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (load_only)
        hipLaunchKernelGGL(fcs_stream_kernel<true>, dim3(grid), dim3(kWgThreads), 0, st, p);
    else
        hipLaunchKernelGGL(fcs_stream_kernel<false>, dim3(grid), dim3(kWgThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_one(const OneArgs &a, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    hipLaunchKernelGGL(fcs_one_kernel, dim3(1), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tx_small(const TxSmallArgs &a, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    hipLaunchKernelGGL(fcs_tx_small_kernel, dim3(a.n), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_small_list(const ListArgs &a, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    hipLaunchKernelGGL(fcs_small_list_kernel, dim3(a.n), dim3(64), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_tx_store(uint8_t *base, uint64_t stride, const uint32_t *len, const uint32_t *crc,
                           uint64_t n, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(tx_store_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, base, stride, len, crc, n);
    return hipGetLastError();
}

}  // namespace fcs
