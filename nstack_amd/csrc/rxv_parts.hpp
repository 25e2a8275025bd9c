// rxv_parts.hpp — device helpers shared by rxv_kernel.hip and txs_kernel.hip: the one's-complement
// folds, the quarter-wave frame walk (Frame, Pos, Geo, Chunk, issue) and the validator's header
// decode. Device code only (included by the .hip translation units).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "rxv_launch.hpp"

namespace rxv {

using fcs::kChunkBytes;
using fcs::kChunkWords;
using fcs::kGroup;
using fcs::kSegBytes;
using fcs::u32x4a4;

__device__ __forceinline__ uint32_t swap16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

// End-around-carry fold to [0, 0xffff]; 0 only for x == 0 (inet_kernel.hip).
__device__ __forceinline__ uint32_t fold64(uint64_t x) {
    uint64_t y = (x & 0xffffffffull) + (x >> 32);
    y = (y & 0xffffu) + (y >> 16);
    y = (y & 0xffffu) + (y >> 16);
    return (uint32_t)((y & 0xffffu) + (y >> 16));
}

// Sum over a 16-lane row; every lane ends with the row's sum.
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror
    return v;
}

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

// What a frame's header decided before its first chunk is summed (uniform over the frame's lanes).
struct Hdr {
    uint32_t bits;    // verdict bits that need no sum
    uint32_t ps;      // L4: accumulator start plus pseudo header; 0 = no L4 checksum to verify
    int cl;           // frame position of the first byte behind the L4 segment (tail mask)
    uint32_t sums;    // this lane's parts, memory grid, folded: bits 0..15 the IP header's sum, bits 16..31
                      // the sum of frame bytes [0, 14 + hlen)
};

// Dword D (0..15) of a 16-lane row's value.
__device__ __forceinline__ uint32_t row_get(uint32_t v, uint32_t D) {
    return (uint32_t)__shfl((int)v, (int)D, kGroup);
}

// The header fields both directions decode (rxv::decode here, txs::decode in txs_kernel.hip), read
// from the row's header dwords: uniform over the frame's lanes.
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

template <bool TRAILER>
__device__ __forceinline__ Hdr decode(const Frame &fr, const Chunk &ch, int j) {
    Hdr h{0u, 0u, 0, 0u};
    const uint32_t F = fr.len, T = TRAILER ? 4u : 0u, r = (uint32_t)fr.start & 3u;
    const HdrWords hw = header_words(fr, ch);
    const uint32_t w12 = hw.w12, src = hw.src, dst = hw.dst;
    const uint32_t hlen = hw.hlen, iplen = hw.iplen, foff = hw.foff, proto = hw.proto;
    // the UDP checksum field, frame bytes 20 + hlen and the next (a multiple of 4: dword (20 + hlen) / 4)
    const uint32_t ud = (20u + hlen) >> 2;   // 5..20
    const uint32_t ua0 = row_get(ch.h0, ud & 15u), ua1 = row_get(ch.h1, ud & 15u);
    const uint32_t ub0 = row_get(ch.h0, (ud + 1u) & 15u), ub1 = row_get(ch.h1, (ud + 1u) & 15u);
    const uint32_t ufield =
        __builtin_amdgcn_alignbyte(ud + 1u < 16u ? ub0 : ub1, ud < 16u ? ua0 : ua1, r) & 0xffffu;

    int che = 0;   // frame position behind the IP header; 0 = no header sum
    if (F < 14u + T) {
        h.bits = kRunt;
    } else if (swap16(w12 & 0xffffu) == 0x0800u) {
        const uint32_t P = F - 14u - T;
        h.bits = kIpv4;
        if (bad_ip_header(hw, P)) {
            h.bits |= kIpBadHdr;
        } else {
            che = 14 + (int)hlen;
            h.bits |= proto << kProtoShift;
            if (iplen != P) h.bits |= kIpBadLen;
            if (foff & 0x3fffu) {
                h.bits |= kFrag;
            } else if (hlen <= iplen && iplen <= P) {
                const uint32_t L = iplen - hlen, l16 = swap16(L);
                const uint32_t a4 = (src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16);
                if (proto == 6u) {          // tcp_checksum(ntohl(src), ntohl(dst), seg, L): htonl() of both
                    if (L < 20u) h.bits |= kL4Short;   // gives back the words as they lie in the header
                    else h.ps = 0xffffu + a4 + 0x0600u + l16;
                } else if (proto == 17u) {  // udp_checksum(seg, L, src, dst): the raw in_addr_t words
                    if (L < 8u) h.bits |= kL4Short;
                    else if (ufield != 0u) h.ps = a4 + 0x1100u + l16;
                } else if (proto == 1u) {   // ip_checksum(msg, L)
                    if (L < 4u) h.bits |= kL4Short;
                    else h.ps = 0xffffu;
                }
                if (h.ps) {
                    h.bits |= kL4Checked;
                    h.cl = 14 + (int)iplen;
                }
            }
        }
    }
    // this lane's two header dwords: byte 0 of dword D at frame position 4 D - r
    const int q0 = 4 * j - (int)r;
    const uint64_t hs = (uint64_t)keep_range(ch.h0, q0, 14, che > 14 ? che : 14) +
                        keep_range(ch.h1, q0 + 64, 14, che > 14 ? che : 14);
    const uint64_t h0 = (uint64_t)keep_range(ch.h0, q0, 0, che) + keep_range(ch.h1, q0 + 64, 0, che);
    h.sums = fold64(hs) | (fold64(h0) << 16);
    return h;
}

}  // namespace rxv
