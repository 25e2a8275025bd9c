// frame_walk.hpp — the quarter-wave frame walk, written once for rxv_kernel.hip, txs_kernel.hip and
// txf_kernel.hip: the frame and chunk geometry (Frame, Pos, Geo, Chunk, issue, next_pos), a chunk's
// words (chunk_words), the front mask, the total and tail sums and their reduction to the frame
// start's word grid, the header-field extraction, the in-register patch of a 16-bit field
// (xor_field), the per-wave count and the two-items-in-flight driver; and for the LDS-DMA pair (rxv_dma_kernel, txs_dma_kernel) the slot geometry and the
// window read. The rules of the walk live here; the kernels add what is their own (verdict; patch
// and stores; header image, padding and stores). One rule is stated twice on purpose: geo_of forms
// the chunk address from the frame's end and not through rel_of, which cost three 64-bit adds per
// chunk. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dispenser.hpp"
#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "ones_fold.hpp"
#include "rxv_launch.hpp"

namespace rxv {

using fcs::kChunkBytes;
using fcs::kChunkWords;
using fcs::kGroup;
using fcs::kSegBytes;
using fcs::u32x4a4;
using ones::fold64;
using ones::row_sum;
using ones::swap16;

// The bytes of dword w (its byte 0 at frame position q0) at positions in [lo, hi), lo <= hi.
__device__ __forceinline__ uint32_t keep_range(uint32_t w, int q0, int lo, int hi) {
    return fcs::clear_low_bits(w, 8 * (lo - q0)) ^ fcs::clear_low_bits(w, 8 * (hi - q0));
}

struct Frame {
    uint64_t start;   // address of the frame's first byte
    uint32_t len;
    uint32_t m;       // segments
};

template <bool VAR>
__device__ __forceinline__ Frame frame_of(const RParams &p, uint64_t f) {
    Frame fr;
    fr.len = VAR ? p.len[f] : p.flen;
    fr.start = p.base + (VAR ? p.off[f] : f * p.stride);
    fr.m = fr.len ? (fr.len + (kSegBytes - 1)) / kSegBytes : 1u;
    return fr;
}

struct Pos {
    uint64_t f;
    uint32_t k;   // segment
    bool act;
    Frame fr;
};

// The grid's first position of this quarter-wave, and the one after c: the frame's next segment,
// or segment 0 of the frame Q (the grid's frame slots) further on.
template <bool VAR>
__device__ __forceinline__ Pos first_pos(const RParams &p, uint64_t f) {
    Pos a;
    a.f = f;
    a.k = 0;
    a.act = f < p.n;
    a.fr = a.act ? frame_of<VAR>(p, f) : Frame{0, 0, 1};
    return a;
}

template <bool VAR>
__device__ __forceinline__ Pos next_pos(const RParams &p, const Pos &c, uint64_t Q) {
    Pos n = c;
    n.k = c.k + 1;
    if (n.k >= c.fr.m) {
        n.f = c.f + Q;
        n.k = 0;
    }
    n.act = c.act && n.f < p.n;
    if (n.act && n.k == 0) n.fr = frame_of<VAR>(p, n.f);
    return n;
}

// Frame position of the first byte of lane j's chunk of segment k: chunks of 96 bytes and segments
// of 1536 are counted back from the frame END (negative in front of the frame).
__device__ __forceinline__ int64_t rel_of(uint32_t len, uint32_t m, uint32_t k, int j) {
    return (int64_t)len - (int64_t)kSegBytes * (int64_t)(m - 1 - k) - (int64_t)kChunkBytes * (j + 1);
}

// Raw loads of one lane chunk (fcs_kernel.hip's Chunk) and, with a frame's first chunk, the two
// header dwords of this lane.
struct Chunk {
    u32x4a4 x[6];
    uint32_t x6;
    uint32_t h0, h1;   // dwords j and j + 16 from floor4(frame start); 0 where outside the frame
    int zr;            // bytes from chunk start to frame start (segment 0); -1 inside; 96 = no data
    uint32_t r;        // chunk start & 3
    int dlead;         // dwords the load window was moved up to stay >= lo4
};

// Where lane j's chunk of segment c.k lies.
struct Geo {
    uint64_t a;    // load address: floor4(chunk start), or lo4 for a lane with nothing to load
    int zr;        // bytes from chunk start to frame start (segment 0); -1 inside; 96 = no data
    uint32_t r;    // chunk start & 3
    int dlead;     // dwords the load window is moved up to stay >= lo4
    bool need;
};

__device__ __forceinline__ Geo geo_of(const RParams &p, const Pos &c, int j) {
    Geo g;
    // the address rel_of's position lies at, formed from the frame's end (whose sum issue() shares)
    const uint64_t end = c.fr.start + c.fr.len;
    const int64_t cstart = (int64_t)end - (int64_t)kSegBytes * (int64_t)(c.fr.m - 1 - c.k) -
                           (int64_t)kChunkBytes * (j + 1);
    const int64_t z = (c.k == 0) ? ((int64_t)c.fr.start - cstart) : -1;
    g.zr = z < -1 ? -1 : (z > kChunkBytes ? kChunkBytes : (int)z);
    g.r = (uint32_t)cstart & 3u;
    g.need = c.act && g.zr < kChunkBytes;
    g.a = g.need ? ((uint64_t)cstart & ~3ull) : p.lo4;
    g.dlead = g.a < p.lo4 ? (int)((p.lo4 - g.a) >> 2) : 0;
    return g;
}

// As fcs::issue_chunk: unconditional loads inside [lo4, hi4) (TINY: guarded dword by dword). The
// header dwords are loaded only where they lie inside [floor4(start), ceil4(end)).
template <bool TINY>
__device__ __forceinline__ void issue(const RParams &p, const Pos &c, int j, Chunk &ch) {
    fcs::LoadPriority lp;
    const Geo g = geo_of(p, c, j);
    ch.zr = g.zr;
    ch.r = g.r;
    ch.dlead = TINY ? 0 : g.dlead;
    ch.h0 = ch.h1 = 0u;
    if (c.act && c.k == 0) {
        const uint64_t ha = (c.fr.start & ~3ull) + 4ull * (uint32_t)j, he = (c.fr.start + c.fr.len + 3) & ~3ull;
        if (ha + 4 <= he) ch.h0 = fcs::gload<uint32_t>(ha);
        if (ha + 68 <= he) ch.h1 = fcs::gload<uint32_t>(ha + 64);
    }
    if (TINY) {
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q <= kChunkWords; q++) {
            const uint64_t ad = g.a + 4 * q;
            d[q] = (g.need && ad >= p.lo4 && ad + 4 <= p.hi4) ? fcs::gload<uint32_t>(ad) : 0u;
        }
#pragma unroll
        for (int q = 0; q < 6; q++) ch.x[q] = u32x4a4{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
        ch.x6 = d[kChunkWords];
        return;
    }
    // a window that starts before lo4 (front lane of a frame at the arena start) is moved up as a
    // whole and shifted back when it is used
    const uint64_t ab = g.a < p.lo4 ? p.lo4 : g.a;
#pragma unroll
    for (int q = 0; q < 6; q++) ch.x[q] = fcs::gload<u32x4a4>(ab + 16 * q);
    ch.x6 = fcs::gload<uint32_t>(ab + ((g.r || g.dlead) ? 96 : 92));
}

// ---- a chunk's words ----
__device__ __forceinline__ void unpack(const u32x4a4 (&x)[6], uint32_t x6, uint32_t (&d)[kChunkWords + 1]) {
#pragma unroll
    for (int q = 0; q < 6; q++) {
        d[4 * q] = x[q].x;
        d[4 * q + 1] = x[q].y;
        d[4 * q + 2] = x[q].z;
        d[4 * q + 3] = x[q].w;
    }
    d[kChunkWords] = x6;
}

// Word i = the four bytes from byte 4 i + r of the 25 loaded dwords.
__device__ __forceinline__ void align_words(const uint32_t (&d)[kChunkWords + 1], uint32_t r, uint32_t (&w)[kChunkWords]) {
#pragma unroll
    for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], r);
}

template <bool TINY>
__device__ __forceinline__ void chunk_words(const Chunk &ch, uint32_t (&w)[kChunkWords]) {
    uint32_t d[kChunkWords + 1];
    unpack(ch.x, ch.x6, d);
    if (!TINY && __any(ch.dlead)) fcs::shift_up(d, ch.dlead);   // arena start only; uniform
    align_words(d, ch.r, w);
}

// Zeroes the zr bytes in front of the frame start. zmax: a uniform bound on zr; words no front lane
// can mask are skipped.
__device__ __forceinline__ void front_mask(uint32_t (&w)[kChunkWords], int zr, int zmax) {
#pragma unroll
    for (int i = 0; i < kChunkWords; i++) {
        if (4 * i < zmax) {
            int t = zr - 4 * i;
            t = t < 0 ? 0 : (t > 4 ? 4 : t);
            w[i] &= (uint32_t)(0xFFFFFFFFull << (8 * t));
        }
    }
}

// ---- CRC (the kernels' LDS holds the FCS engine's table blob) ----
__device__ __forceinline__ fcs::KParams tables_of(const uint32_t *blob) {   // for fcs::stage_tables
    fcs::KParams kp{};
    kp.blob = blob;
    return kp;
}

// The frame's CRC register after one more chunk: the frame's first chunk starts it (INV start in
// the lane that holds the frame start), a later segment's advances it by A_1536.
__device__ __forceinline__ uint32_t crc_step(const uint8_t *lds, uint32_t s, const uint32_t (&w)[kChunkWords], bool first,
                                             int zr, uint32_t tb0, uint32_t tb1) {
    uint32_t x0 = 0;
    if (first) x0 = fcs::inv_start(lds, zr);
    const uint32_t rr = fcs::chunk_crc(lds, w, x0, tb0, tb1);
    return first ? rr : fcs::uniform_shift<fcs::kLdsJump>(lds, s, rr);
}

// The frame's register from its lanes' (rows at their frame's last chunk; 0 in the others).
__device__ __forceinline__ uint32_t crc_join(const uint8_t *lds, uint32_t s, bool last, uint32_t lanebase) {
    return fcs::row_xor(last ? fcs::lane_shift(lds, s, lanebase) : 0u);
}

// ---- sums ----
// Every word into the total; words holding bytes from frame position cl on (the bytes behind the L4
// segment; none without ps) also into the tail, under a mask, only in the 6-word blocks some lane
// of the wave has such bytes in. dt: cl relative to the chunk's first byte, clamped to [-4, 100]
// by add_sums (below); the masks clamp again.
__device__ __forceinline__ void add_sums_cut(const uint32_t (&w)[kChunkWords], int dt, uint64_t &tot, uint64_t &tail) {
    uint64_t a = 0;
#pragma unroll
    for (int i = 0; i < kChunkWords; i += 2) a += (uint64_t)w[i] + w[i + 1];
    tot += a;
    uint64_t b = 0;
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
        if (__any(dt < 24 * (blk + 1))) {
#pragma unroll
            for (int i = 6 * blk; i < 6 * blk + 6; i++) b += fcs::clear_low_bits(w[i], 8 * (dt - 4 * i));
        }
    }
    tail += b;
}

// rel: frame position of the chunk's first byte. rel_of's int64_t in the general walk (the clamp
// keeps what follows inside an int); an int where it is known to fit one, the LDS-DMA kernels' loop
// invariant: in 64 bits its sign word costs txs_dma_kernel the one register it has not got.
__device__ __forceinline__ void add_sums(const uint32_t (&w)[kChunkWords], int64_t rel, int cl, uint32_t ps,
                                         uint64_t &tot, uint64_t &tail) {
    const int64_t dl = (int64_t)cl - rel;
    add_sums_cut(w, !ps ? kChunkBytes + 4 : (dl < -4 ? -4 : (dl > kChunkBytes + 4 ? kChunkBytes + 4 : (int)dl)), tot, tail);
}
__device__ __forceinline__ void add_sums(const uint32_t (&w)[kChunkWords], int rel, int cl, uint32_t ps, uint64_t &tot,
                                         uint64_t &tail) {
    const int dl = cl - rel;
    add_sums_cut(w, !ps ? kChunkBytes + 4 : (dl < -4 ? -4 : (dl > kChunkBytes + 4 ? kChunkBytes + 4 : dl)), tot, tail);
}

// This lane's parts of the header sums from its two header dwords (byte 0 of dword D at frame
// position 4 D - r), memory grid, folded: bits 0..15 the IP header's sum [14, che), bits 16..31 the
// sum of frame bytes [0, che). che = 0: no header sum.
__device__ __forceinline__ uint32_t header_sums(const Chunk &ch, int j, uint32_t r, int che) {
    const int q0 = 4 * j - (int)r;
    const uint64_t hs = (uint64_t)keep_range(ch.h0, q0, 14, che > 14 ? che : 14) +
                        keep_range(ch.h1, q0 + 64, 14, che > 14 ? che : 14);
    const uint64_t h0 = (uint64_t)keep_range(ch.h0, q0, 0, che) + keep_range(ch.h1, q0 + 64, 0, che);
    return fold64(hs) | (fold64(h0) << 16);
}

// The frame's four sums (row-uniform), each on the frame start's word grid: the end grid (total,
// tail) differs for an odd length, memory's (header_sums' parts) for an odd start.
struct Sums {
    uint32_t tot_s, tail_s;   // the frame; its bytes from cl on
    uint32_t hdr_s, head_s;   // the IP header; frame bytes [0, 14 + hlen)
};

__device__ __forceinline__ Sums reduce_sums(uint64_t tot, uint64_t tail, uint32_t hsums, bool odd_len, bool odd_start) {
    const uint32_t te = fold64(row_sum(fold64(tot))), ta = fold64(row_sum(fold64(tail)));
    const uint32_t hm = fold64(row_sum(hsums & 0xffffu)), h0 = fold64(row_sum(hsums >> 16));
    return Sums{odd_len ? swap16(te) : te, odd_len ? swap16(ta) : ta, odd_start ? swap16(hm) : hm,
                odd_start ? swap16(h0) : h0};
}

// ---- a 16-bit field in a chunk's words (the TX kernels patch checksum fields in registers) ----
constexpr int kNoField = 1 << 20;   // a chunk byte offset no chunk has

// XORs the 16-bit value `delta` (its low byte first) into the chunk words at chunk byte offset b,
// by bytes: b = -1 reaches only the second byte (word 0), b = 95 only the first; any other b outside
// [0, 95) does nothing. Only the 6-word blocks some lane of the wave has such bytes in are touched.
__device__ __forceinline__ void xor_field(uint32_t (&w)[kChunkWords], int b, uint32_t delta) {
    const bool in = b >= -1 && b < kChunkBytes;
    const int iw = b >> 2;   // -1 for b = -1
    const uint64_t P = (uint64_t)delta << (8 * (b & 3));
    const uint32_t P0 = in ? (uint32_t)P : 0u, P1 = in ? (uint32_t)(P >> 32) : 0u;
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
        if (__any(in && iw + 1 >= 6 * blk && iw < 6 * blk + 6)) {
#pragma unroll
            for (int i = 6 * blk; i < 6 * blk + 6; i++) w[i] ^= (i == iw ? P0 : 0u) ^ (i == iw + 1 ? P1 : 0u);
        }
    }
}

// ---- the per-wave count (wb = fcs::wave_bad of the kernel's LDS) ----
__device__ __forceinline__ void count_bad(uint64_t *wb, int lane, bool bad) {
    const uint64_t mb = __ballot(bad);
    if (mb != 0 && lane == 0) *wb += (uint64_t)__popcll(mb);
}

__device__ __forceinline__ void flush_bad(const uint64_t *wb, int lane, unsigned long long *out) {
    if (out != nullptr && lane == 0) {
        const uint64_t b = *wb;
        if (b) atomicAdd(out, (unsigned long long)b);
    }
}

// ---- the driver: two items in flight per lane, one processed while the other's loads are
// outstanding. CH: the kernel's chunk registers; next(pos) -> pos, issue(pos, CH &), process(pos, CH). ----
template <class CH, class P, class Next, class Issue, class Process>
__device__ __forceinline__ void two_in_flight(P A, const Next &next, const Issue &issue, const Process &process) {
    P B;
    CH CA, CB;
    issue(A, CA);
    while (__any(A.act)) {
        B = next(A);
        issue(B, CB);
        process(A, CA);
        if (!__any(B.act)) break;
        A = next(B);
        issue(A, CA);
        process(B, CB);
    }
}

// Dword D (0..15) of a 16-lane row's value.
__device__ __forceinline__ uint32_t row_get(uint32_t v, uint32_t D) {
    return (uint32_t)__shfl((int)v, (int)D, kGroup);
}

// The header fields both directions decode (rxv::decode in rxv_kernel.hip, txs::decode in
// txs_kernel.hip), read from the row's header dwords: uniform over the frame's lanes.
struct HdrWords {
    uint32_t w12;            // frame bytes 12..15: ethertype, vhl, tos
    uint32_t w24;            // frame bytes 24..27: ip_csum, src (low half)
    uint32_t src, dst;       // the address words as they lie in the header
    uint32_t vhl, hlen, iplen, foff, proto;
};

__device__ __forceinline__ HdrWords header_words(const Frame &fr, const Chunk &ch) {
    HdrWords o;
    const uint32_t r = (uint32_t)fr.start & 3u;
    // dwords 3..9 from floor4(start) hold frame bytes 12..33 at any alignment
    uint32_t g[7];
#pragma unroll
    for (int q = 0; q < 7; q++) g[q] = row_get(ch.h0, 3u + q);
    o.w12 = __builtin_amdgcn_alignbyte(g[1], g[0], r);                  // ethertype, vhl, tos
    const uint32_t w16 = __builtin_amdgcn_alignbyte(g[2], g[1], r);   // ip_len, id
    const uint32_t w20 = __builtin_amdgcn_alignbyte(g[3], g[2], r);   // foff, ttl, proto
    o.w24 = __builtin_amdgcn_alignbyte(g[4], g[3], r);
    const bool up = r >= 2;                                           // bytes 26.. start in dword 7
    o.src = __builtin_amdgcn_alignbyte(up ? g[5] : g[4], up ? g[4] : g[3], (r + 2u) & 3u);
    o.dst = __builtin_amdgcn_alignbyte(up ? g[6] : g[5], up ? g[5] : g[4], (r + 2u) & 3u);
    o.vhl = (o.w12 >> 16) & 0xffu;
    o.hlen = (o.vhl & 0x0fu) * 4u;
    o.iplen = swap16(w16 & 0xffffu);
    o.foff = swap16(w20 & 0xffffu);
    o.proto = w20 >> 24;
    return o;
}

// The validator's rule 4: the IPv4 header of a frame with P payload bytes cannot be used.
__device__ __forceinline__ bool bad_ip_header(const HdrWords &hw, uint32_t P) {
    return P < 20u || (hw.vhl & 0x40u) != 0x40u || hw.hlen < 20u || hw.hlen > P;
}

// ---------------------------------------------------------------------------------------------
// The LDS-DMA pair (rxv_dma_kernel, txs_dma_kernel): fcs_dma_kernel's load form. A wave item is
// four consecutive frames of a fixed stride that fit a 6 KiB slot (fcs::fixed_dma); items come
// from the work dispenser.
// ---------------------------------------------------------------------------------------------
struct DmaSlots {
    const RParams &p;
    const uint8_t *slot;   // this wave's slot
    int wave, lane;
    uint64_t lo16, smax;   // first and last slot source inside the arena

    __device__ __forceinline__ DmaSlots(const RParams &p_, const uint8_t *lds, int wave_, int lane_)
        : p(p_), slot(lds + fcs::kDmaRing + (uint32_t)wave_ * fcs::kDmaItemBytes), wave(wave_), lane(lane_),
          lo16(p_.lo4 & ~15ull), smax(((p_.hi4 + 15) & ~15ull) - fcs::kDmaItemBytes) {}
    __device__ __forceinline__ fcs::Dispenser dispenser() const {
        constexpr int kWaves = kDmaThreads / 64;
        return fcs::Dispenser(p.ctr, (p.n + 3) >> 2, (uint64_t)gridDim.x * kWaves,
                              (uint64_t)blockIdx.x * kWaves + (uint64_t)wave, lane, 100, 4, 64);
    }
    __device__ __forceinline__ uint64_t item_start(uint64_t i) const { return p.base + 4 * i * p.stride; }
    // the 16-B piece an item's slot starts at, kept inside the arena
    __device__ __forceinline__ uint64_t slot_src(uint64_t S) const {
        const uint64_t a = S & ~15ull;
        return a < lo16 ? lo16 : (a > smax ? smax : a);
    }
    __device__ __forceinline__ void dma_of(uint64_t i) const {
        const uint64_t S = item_start(i), sn = slot_src(S);
        const uint64_t e = S + 3 * p.stride + p.flen + 4 - sn;
        fcs::dma_item(slot, sn, lane, (uint32_t)(e < (uint64_t)fcs::kDmaItemBytes ? e : (uint64_t)fcs::kDmaItemBytes));
    }
};

// Frame g (the lane's quarter) of item `it`, once its DMA has landed: lane c's window, the 25 dwords from rel (frame
// position of the window's first byte) rounded down to a dword, r the bytes to shift them by; the
// frame; and the lane's header dwords c and c + 16 from floor4(frame start) in the slot. A frame
// past the batch's end (last item) works on the item's first frame: nothing outside the slot is read.
// Returns the frame's index in the batch.
__device__ __forceinline__ uint64_t dma_window(const DmaSlots &G, uint64_t it, int g, int c, int rel,
                                           uint32_t (&d)[kChunkWords + 1], uint32_t &r, Frame &fr, Chunk &ch) {
    const RParams &p = G.p;
    const uint64_t f = 4 * it + (uint64_t)g;
    const uint64_t S = G.item_start(it), src = G.slot_src(S);
    __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's slot DMA has landed
    const uint64_t goff = f < p.n ? (uint64_t)g * p.stride : 0ull;
    const int64_t x = (int64_t)(S - src + goff) + rel;   // window start within the slot
    r = (uint32_t)x & 3u;
    const uint32_t *wp = reinterpret_cast<const uint32_t *>(G.slot + (x & ~3ll));
#pragma unroll
    for (int q = 0; q < kChunkWords; q++) d[q] = wp[q];
    {   // the 25th dword matters only when r != 0; clamped so the slot is never read past its end
        const uint64_t a24 = (uint64_t)(wp + kChunkWords), lim = (uint64_t)(G.slot + fcs::kDmaItemBytes - 4);
        d[kChunkWords] = *reinterpret_cast<const uint32_t *>(a24 < lim ? a24 : lim);
    }
    fr.start = S + goff;   // slots start at 16-B pieces: same low address bits
    fr.len = p.flen;
    fr.m = 1;
    const uint32_t hb = (uint32_t)(S - src + goff) & ~3u;
    const uint32_t *hp = reinterpret_cast<const uint32_t *>(G.slot + hb);
    ch.h0 = hp[c];
    ch.h1 = hp[c + 16];
    return f;
}

}  // namespace rxv
