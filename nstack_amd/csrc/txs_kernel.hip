// txs_kernel.hip — one-pass TX sealing for gfx950: the IPv4 header checksum, the TCP / UDP / ICMP
// checksum and the FCS of every frame of a batch, computed from ONE read of its bytes and stored in
// place (include/nstack_txs.h has the rules and the reference lines they restate). The mirror image
// of rxv_kernel.hip, whose frame walk, loads, sums and CRC forms it shares (rxv_parts.hpp,
// fcs_crc.hpp): a QUARTER-WAVE per frame, lane j owns the 96-byte chunk that ends 96 j bytes before
// the frame end, longer frames are walked in 1536-byte segments counted from the frame END, lane l
// also holds dwords l and l + 16 of the frame's first 128 bytes.
//
// What differs from validation:
//   * The fields' old content is ignored. All three fields lie in frame bytes [24, 92), at even
//     frame positions, inside the header dwords: the old IP and L4 field values are read from them
//     (ds_bpermute, as the validator reads the UDP field) and leave the sums in one's-complement
//     arithmetic on the frame start's word grid, where the head and tail parts are subtracted too:
//       IP  = ~fold(0xffff + [14, 14 + hlen) - old_ip)
//       L4  = ~fold(pseudo + total - [0, 14 + hlen) - [14 + ip_len, F) - old_l4)
//   * The CRC must be that of the PATCHED bytes, but the L4 value needs the whole frame's sum.
//       - A single-segment frame (F <= 1536) has all its words in registers at once: the sums are
//         reduced first, delta = new ^ old of each field is XORed into the words (by bytes: the
//         words are aligned to the frame END, so a field straddles two words when F is odd and two
//         lanes' chunks when F == q + 1 (mod 96)), then the chains run. An ordering dependency only.
//       - A multi-segment frame cannot wait. The CRC is linear: the patched frame's CRC register is
//         the raw one XOR the register of a frame that is zero except for the deltas. The 68 bytes
//         [24, 92) touch at most two consecutive chunks, which belong to two different lanes, so at
//         the frame's last chunk each lane builds the one delta chunk it owns (possibly in
//         different segments: a field can lie astride segments 0 and 1), runs the two chains over
//         it once more, advances the result by A_1536 once per segment behind it and XORs it into
//         its register before the lane shift. Cost: one extra chunk pass per multi-segment frame
//         plus m - 1 (or m - 2) table shifts of 8 LDS reads.
//   * Stores are plain per-lane stores: byte stores for the fields and the FCS (frame starts have
//     any alignment), lane 15 the status word and the fields record, lane 14 the IP field, lane 13
//     the L4 field, lanes 0..3 one FCS byte each. A neighbouring wave may load a 16-byte piece that
//     holds bytes this wave is writing (the end of the frame in front, the FCS place behind): it
//     masks those bytes, as the validator does, so no byte that is written is interpreted by anyone
//     but the frame's own quarter-wave, which has loaded it before. Read bounds are rxv_kernel's.
// txs_dma_kernel (below) is the same arithmetic on rxv_dma_kernel's load form for fixed strides of
// 1496..1524-B frames (always single-segment: patched in registers); txs::route decides.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "dispenser.hpp"
#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "rxv_parts.hpp"
#include "txs_launch.hpp"

namespace txs {

using fcs::kChunkBytes;
using fcs::kChunkWords;
using fcs::kGroup;
using fcs::kSegBytes;
using rxv::Chunk;
using rxv::fold64;
using rxv::Frame;
using rxv::keep_range;
using rxv::Pos;
using rxv::row_get;
using rxv::row_sum;
using rxv::RParams;
using rxv::swap16;

constexpr int kNoField = 1 << 20;   // a chunk byte offset no chunk has

// What a frame's header decided before its first chunk is summed (uniform over the frame's lanes).
struct THdr {
    uint32_t bits;    // status bits that need no sum
    uint32_t ps;      // L4: accumulator start plus pseudo header; 0 = no L4 sum
    uint32_t old;     // the fields' old content, words of the frame start's grid: IP | L4 << 16
    uint32_t sums;    // this lane's parts, memory grid, folded: bits 0..15 the IP header's sum, bits 16..31
                      // the sum of frame bytes [0, 14 + hlen) (both with the old field content)
    int cl;           // frame position of the first byte behind the L4 segment (tail mask)
    int che;          // frame position behind the IP header; 0 = no IP checksum to write
    int ql4;          // frame position of the L4 checksum field; 0 = none to write
};

__device__ __forceinline__ THdr decode(const Frame &fr, const Chunk &ch, int j, uint32_t flags) {
    THdr h{0u, 0u, 0u, 0u, 0, 0, 0};
    const uint32_t F = fr.len, r = (uint32_t)fr.start & 3u;
    const rxv::HdrWords hw = rxv::header_words(fr, ch);   // the validator's field extraction
    const uint32_t w12 = hw.w12, w24 = hw.w24, src = hw.src, dst = hw.dst;
    const uint32_t hlen = hw.hlen, iplen = hw.iplen, foff = hw.foff, proto = hw.proto;

    if (F < 14u) {
        h.bits = kRunt;
    } else if (swap16(w12 & 0xffffu) == 0x0800u) {
        const uint32_t P = F - 14u;
        h.bits = kIpv4;
        if (rxv::bad_ip_header(hw, P)) {   // exactly the validator's rule 4
            h.bits |= kIpBadHdr;
        } else {
            h.che = 14 + (int)hlen;
            h.bits |= (proto << kProtoShift) | kIpCsumSet;
            h.old = w24 & 0xffffu;
            const bool badlen = iplen < hlen || iplen > P;
            if (badlen) h.bits |= kIpBadLen;
            if (foff & 0x3fffu) h.bits |= kFrag;
            if (!badlen && !(foff & 0x3fffu)) {
                const uint32_t L = iplen - hlen, l16 = swap16(L);
                const uint32_t a4 = (src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16);
                if (proto == 6u) {          // tcp_checksum(ntohl(src), ntohl(dst), seg, L)
                    if (L < 20u) h.bits |= kL4Short;
                    else h.ps = 0xffffu + a4 + 0x0600u + l16, h.ql4 = h.che + 16;
                } else if (proto == 17u) {  // udp_checksum(seg, L, src, dst): the raw in_addr_t words
                    if (L < 8u) h.bits |= kL4Short;
                    else h.ps = (flags & kFlagUdpZero) ? 0u : a4 + 0x1100u + l16, h.ql4 = h.che + 6;
                } else if (proto == 1u) {   // ip_checksum(msg, L)
                    if (L < 4u) h.bits |= kL4Short;
                    else h.ps = 0xffffu, h.ql4 = h.che + 2;
                }
                if (h.ps) {
                    h.bits |= kL4CsumSet;
                    h.cl = 14 + (int)iplen;
                }
            }
        }
    }
    // the L4 field's old content: frame bytes ql4, ql4 + 1 from the dwords that hold frame bytes
    // 4 D .. 4 D + 7, D = ql4 / 4 (5..22)
    {
        const uint32_t D = (uint32_t)h.ql4 >> 2;
        const uint32_t a0 = row_get(ch.h0, D & 15u), a1 = row_get(ch.h1, D & 15u);
        const uint32_t b0 = row_get(ch.h0, (D + 1u) & 15u), b1 = row_get(ch.h1, (D + 1u) & 15u);
        const uint32_t wd = __builtin_amdgcn_alignbyte(D + 1u < 16u ? b0 : b1, D < 16u ? a0 : a1, r);
        if (h.ql4) h.old |= ((h.ql4 & 2) ? wd >> 16 : wd & 0xffffu) << 16;
    }
    // this lane's two header dwords: byte 0 of dword D at frame position 4 D - r
    const int q0 = 4 * j - (int)r, che = h.che;
    const uint64_t hs = (uint64_t)keep_range(ch.h0, q0, 14, che > 14 ? che : 14) +
                        keep_range(ch.h1, q0 + 64, 14, che > 14 ? che : 14);
    const uint64_t h0 = (uint64_t)keep_range(ch.h0, q0, 0, che) + keep_range(ch.h1, q0 + 64, 0, che);
    h.sums = fold64(hs) | (fold64(h0) << 16);
    return h;
}

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

// The values to write, from the reduced sums (row-uniform).
struct Seal {
    uint32_t ip, l4;     // the uint16 values as stored (low byte at the lower address)
    uint32_t dip, dl4;   // new ^ old; 0 where nothing is written
};

__device__ __forceinline__ Seal seal_of(const THdr &H, uint64_t tot, uint64_t tail, bool odd_len, bool odd_start) {
    Seal z{0u, 0u, 0u, 0u};
    const uint32_t te = fold64(row_sum(fold64(tot))), ta = fold64(row_sum(fold64(tail)));
    const uint32_t hm = fold64(row_sum(H.sums & 0xffffu)), h0 = fold64(row_sum(H.sums >> 16));
    // to the frame start's word grid: the end grid differs for an odd length, memory's for an odd start
    const uint32_t tot_s = odd_len ? swap16(te) : te, tail_s = odd_len ? swap16(ta) : ta;
    const uint32_t hdr_s = odd_start ? swap16(hm) : hm, head_s = odd_start ? swap16(h0) : h0;
    const uint32_t oip = H.old & 0xffffu, ol4 = H.old >> 16;
    if (H.che) {
        z.ip = ~fold64(0xffffull + hdr_s + (0xffffu - oip)) & 0xffffu;
        z.dip = z.ip ^ oip;
    }
    if (H.ql4) {
        if (H.ps) {
            const uint64_t l4 = (uint64_t)H.ps + tot_s + (0xffffu - head_s) + (0xffffu - tail_s) + (0xffffu - ol4);
            z.l4 = ~fold64(l4) & 0xffffu;
            if (z.l4 == 0u && ((H.bits >> kProtoShift) & 0xffu) == 17u) z.l4 = 0xffffu;   // RFC 768
        }
        z.dl4 = z.l4 ^ ol4;
    }
    return z;
}

// The frame's stores (the header comment has who stores what): what the sums decided, and, once the
// chains have run, the FCS. The first part does not wait for the CRC, so nothing but the frame's
// address stays live across the chains.
__device__ __forceinline__ void store_sums(const TParams &tp, bool st, int j, uint64_t f, uint64_t start,
                                           const THdr &H, const Seal &z, uint32_t v) {
    if (!st) return;
    uint8_t *fp = reinterpret_cast<uint8_t *>(start);
    if (j == 15) {
        if (tp.r.verdict != nullptr) tp.r.verdict[f] = v;
        if (tp.fields != nullptr) reinterpret_cast<uint32_t *>(tp.fields + f)[0] = z.ip | ((H.ps ? z.l4 : 0u) << 16);
    }
    if (j == 14 && H.che) {
        fp[24] = (uint8_t)z.ip;
        fp[25] = (uint8_t)(z.ip >> 8);
    }
    if (j == 13 && H.ql4) {
        fp[H.ql4] = (uint8_t)z.l4;
        fp[H.ql4 + 1] = (uint8_t)(z.l4 >> 8);
    }
}

template <bool FCSW>
__device__ __forceinline__ void store_fcs(const TParams &tp, bool st, int j, uint64_t f, uint64_t start, uint32_t F,
                                          uint32_t crc) {
    if (!st) return;
    if (j == 15 && tp.fields != nullptr) reinterpret_cast<uint32_t *>(tp.fields + f)[1] = FCSW ? crc : 0u;
    if (FCSW && j < 4) reinterpret_cast<uint8_t *>(start)[(uint64_t)F + (uint32_t)j] = (uint8_t)(crc >> (8 * j));
}

// Two independent 12-word chains over a chunk, merged with A_48 (fcs_kernel.hip).
__device__ __forceinline__ uint32_t chunk_crc(const uint8_t *lds, const uint32_t (&w)[kChunkWords], uint32_t x0,
                                              uint32_t tb0, uint32_t tb1) {
    uint32_t xa = x0 ^ w[0], xb = w[12];
#pragma unroll
    for (int i = 0; i < 12; i++) {
        xa = fcs::step4(lds, xa, i < 11 ? w[i + 1] : 0u, tb0, tb1);
        xb = fcs::step4(lds, xb, i < 11 ? w[13 + i] : 0u, tb0, tb1);
    }
    return fcs::uniform_shift<fcs::kLdsH48>(lds, xa, xb);
}

template <bool VAR, bool FCSW, bool TINY, int NT>
__global__ __launch_bounds__(NT, 1) void txs_kernel(TParams tp) {
    const RParams &p = tp.r;
    // without the CRC only the per-wave counters live in LDS
    constexpr uint32_t kBad = FCSW ? fcs::kLdsBad : 0u;
    __shared__ __attribute__((aligned(16))) uint8_t lds[FCSW ? fcs::kLdsBytes : 16 * 8];
    if (FCSW) {
        fcs::KParams kp{};
        kp.blob = p.blob;
        fcs::stage_tables<NT>(kp, lds);
    }
    fcs::init_bad<kBad>(lds);
    const int lane = threadIdx.x & 63, j = lane & (kGroup - 1);
    uint32_t tb0, tb1;
    fcs::table_bases(lane, tb0, tb1);
    const uint32_t lanebase = fcs::kLdsLane | ((uint32_t)(lane & 31) * 4u);
    const uint64_t Q = (uint64_t)gridDim.x * (NT / kGroup);   // frame slots in the grid

    auto next = [&](const Pos &c) -> Pos {
        Pos n = c;
        n.k = c.k + 1;
        if (n.k >= c.fr.m) {
            n.f = c.f + Q;
            n.k = 0;
        }
        n.act = c.act && n.f < p.n;
        if (n.act && n.k == 0) n.fr = rxv::frame_of<VAR>(p, n.f);
        return n;
    };

    // per-frame state, carried over the frame's segments
    uint32_t s = 0;            // CRC register
    uint64_t tot = 0, tail = 0;
    THdr H{0u, 0u, 0u, 0u, 0, 0, 0};

    auto process = [&](const Pos &c, const Chunk &ch) {
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q < 6; q++) {
            d[4 * q] = ch.x[q].x;
            d[4 * q + 1] = ch.x[q].y;
            d[4 * q + 2] = ch.x[q].z;
            d[4 * q + 3] = ch.x[q].w;
        }
        d[kChunkWords] = ch.x6;
        if (!TINY && __any(ch.dlead)) fcs::shift_up(d, ch.dlead);   // arena start only; uniform
        uint32_t w[kChunkWords];
#pragma unroll
        for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], ch.r);
        const bool first = c.k == 0;
        if (__any(first)) {   // a frame's first chunk: its header fields
            const THdr hn = decode(c.fr, ch, j, tp.flags);
            if (first) {
                H = hn;
                if (!c.act) H = THdr{0u, 0u, 0u, 0u, 0, 0, 0};
                tot = tail = 0;
            }
        }
        if (first) {   // the front mask
#pragma unroll
            for (int i = 0; i < kChunkWords; i++) {
                if (4 * i < (int)p.zmax) {   // uniform bound: words no front lane can mask are skipped
                    int t = ch.zr - 4 * i;
                    t = t < 0 ? 0 : (t > 4 ? 4 : t);
                    w[i] &= (uint32_t)(0xFFFFFFFFull << (8 * t));
                }
            }
        }
        // ---- sums (rxv_kernel): every word into the total; words holding bytes from cl on also into the tail ----
        {
            uint64_t a = 0;
#pragma unroll
            for (int i = 0; i < kChunkWords; i += 2) a += (uint64_t)w[i] + w[i + 1];
            tot += a;
            const int64_t rel = (int64_t)c.fr.len - (int64_t)kSegBytes * (int64_t)(c.fr.m - 1 - c.k) -
                                (int64_t)kChunkBytes * (j + 1);
            const int64_t dl = (int64_t)H.cl - rel;
            const int dt = !H.ps ? kChunkBytes + 4 : (dl < -4 ? -4 : (dl > kChunkBytes + 4 ? kChunkBytes + 4 : (int)dl));
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
        // ---- the frame's last chunk: the values; a single-segment frame is patched in its registers ----
        const bool last = c.act && c.k + 1 == c.fr.m;
        Seal z{0u, 0u, 0u, 0u};
        if (__any(last)) {
            z = seal_of(H, tot, tail, c.fr.len & 1u, c.fr.start & 1ull);
            if (FCSW) {
                const bool one = last && first;
                // frame position of the chunk's first byte; used for a single segment only (<= 1536 - 96)
                const int rel = (int)((int64_t)c.fr.len - (int64_t)kChunkBytes * (j + 1));
                xor_field(w, one ? 24 - rel : kNoField, z.dip);
                xor_field(w, one && H.ql4 ? H.ql4 - rel : kNoField, z.dl4);
            }
        }
        // ---- CRC: two independent 12-word chains, merged with A_48 (fcs_kernel.hip) ----
        if (FCSW) {
            uint32_t x0 = 0;
            if (first) {
                const int zi = ch.zr < 0 ? 0 : (ch.zr > kChunkBytes - 1 ? kChunkBytes - 1 : ch.zr);
                const uint32_t iv = fcs::lds_rd(lds, fcs::kLdsInv + 4u * (uint32_t)zi);
                x0 = (ch.zr >= 0 && ch.zr < kChunkBytes) ? iv : 0u;
            }
            const uint32_t rr = chunk_crc(lds, w, x0, tb0, tb1);
            s = first ? rr : fcs::uniform_shift<fcs::kLdsJump>(lds, s, rr);
        }
        if (__any(last)) {
            uint32_t v = H.bits, crc = 0u;
            if (FCSW) {
                // a multi-segment frame: the deltas' own CRC register, from the one chunk of this lane
                // that holds bytes of [24, 92) (chunks counted from the frame end; lane = chunk & 15)
                const bool mc = last && !first && (z.dip | z.dl4) != 0u;
                if (__any(mc)) {
                    const uint32_t F = c.fr.len;   // > 1536 where mc
                    const uint32_t chi = mc ? (F - 25u) / (uint32_t)kChunkBytes : 0u;
                    const uint32_t clo = mc ? (F - 92u) / (uint32_t)kChunkBytes : 0u;
                    const bool own_hi = mc && (int)(chi & 15u) == j, own_lo = mc && (int)(clo & 15u) == j;
                    const uint32_t ci = own_hi ? chi : clo;
                    const bool own = own_hi || own_lo;
                    const int rel = (int)((int64_t)F - (int64_t)kChunkBytes * ((int64_t)ci + 1));
                    uint32_t dw[kChunkWords];
#pragma unroll
                    for (int i = 0; i < kChunkWords; i++) dw[i] = 0u;
                    xor_field(dw, own ? 24 - rel : kNoField, z.dip);
                    xor_field(dw, own && H.ql4 ? H.ql4 - rel : kNoField, z.dl4);
                    uint32_t rd = chunk_crc(lds, dw, 0u, tb0, tb1);
                    const uint32_t cnt = own ? ci >> 4 : 0u;   // segments behind the chunk's
                    for (uint32_t t = 0; __any(t < cnt); t++) {
                        const uint32_t nx = fcs::uniform_shift<fcs::kLdsJump>(lds, rd, 0u);
                        rd = t < cnt ? nx : rd;
                    }
                    s ^= own ? rd : 0u;
                }
                uint32_t x = last ? fcs::lane_shift(lds, s, lanebase) : 0u;
                x = fcs::row_xor(x);
                crc = c.fr.len ? ~x : 0u;
                v |= kFcsSet;
            }
            store_sums(tp, last, j, c.f, c.fr.start, H, z, v);
            store_fcs<FCSW>(tp, last, j, c.f, c.fr.start, c.fr.len, crc);
            const uint64_t mb = __ballot(last && j == 15 && (v & p.bad_mask) != 0u);
            if (mb != 0 && lane == 0) *fcs::wave_bad<kBad>(lds) += (uint64_t)__popcll(mb);
        }
    };

    Pos A, B;
    A.f = (uint64_t)blockIdx.x * (NT / kGroup) + threadIdx.x / kGroup;
    A.k = 0;
    A.act = A.f < p.n;
    A.fr = A.act ? rxv::frame_of<VAR>(p, A.f) : Frame{0, 0, 1};
    Chunk CA, CB;
    rxv::issue<TINY>(p, A, j, CA);
    // two items in flight per lane: process one while the other's loads are outstanding
    while (__any(A.act)) {
        B = next(A);
        rxv::issue<TINY>(p, B, j, CB);
        process(A, CA);
        if (!__any(B.act)) break;
        A = next(B);
        rxv::issue<TINY>(p, A, j, CA);
        process(B, CB);
    }
    if (p.bad != nullptr && lane == 0) {
        const uint64_t b = *fcs::wave_bad<kBad>(lds);
        if (b) atomicAdd(p.bad, (unsigned long long)b);
    }
}

// ---------------------------------------------------------------------------------------------
// Fixed-stride batches through LDS (txs_dma_kernel): rxv_dma_kernel's load form (four-frame wave
// items in 6 KiB slots by global_load_lds, the next item's DMA in flight, items from the work
// dispenser, 16 waves per CU), windows, sums and CRC. Every frame is a single segment: the sums are
// reduced, the deltas XORed into the window registers (the fields lie in lanes 15 and 14, whose
// windows neither overlap nor carry a masked overlap word), then the chains run. The slot DMA of
// the next item is issued before this item's stores: it can hold only bytes in front of its first
// frame or behind its last that are being written, and those are masked.
// ---------------------------------------------------------------------------------------------
template <bool FCSW>
__global__ __launch_bounds__(kDmaThreads, 1) void txs_dma_kernel(TParams tp) {
    using namespace fcs;
    const RParams &p = tp.r;
    constexpr int kWaves = kDmaThreads / 64;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDmaRing + kWaves * kDmaItemBytes];
    const int tid = threadIdx.x;
    if (FCSW) {
        KParams kp{};
        kp.blob = p.blob;
        stage_dma_tables<kDmaThreads>(kp, lds, tid);
    }
    init_bad<kDmaBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const int c = lane & (kGroup - 1);     // chunk index back from the frame end
    const int g = lane >> 4;               // frame of the item
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint8_t *slot = lds + kDmaRing + (uint32_t)wave * kDmaItemBytes;

    // loop invariants: the window's place in the frame, leading bytes to mask
    const uint32_t ec = dma_end_off(c);
    const int rel = (int)p.flen - (int)ec - kChunkBytes;   // frame position of the window's first byte (>= -28)
    const int zc = (c == kGroup - 1) ? (int)(kDmaCover - p.flen) : (dma_short_lane(c) ? 4 : 0);

    const uint64_t lo16 = p.lo4 & ~15ull;
    const uint64_t smax = ((p.hi4 + 15) & ~15ull) - kDmaItemBytes;   // last slot start inside the arena
    auto slot_src = [&](uint64_t S) {
        const uint64_t a = S & ~15ull;
        return a < lo16 ? lo16 : (a > smax ? smax : a);
    };
    constexpr uint64_t kEnd = Dispenser::kEnd;
    Dispenser D(p.ctr, (p.n + 3) >> 2, (uint64_t)gridDim.x * kWaves,
                (uint64_t)blockIdx.x * kWaves + (uint64_t)wave, lane, 100, 4, 64);
    auto item_start = [&](uint64_t i) { return p.base + 4 * i * p.stride; };
    auto dma_of = [&](uint64_t i) {
        const uint64_t S = item_start(i), sn = slot_src(S);
        const uint64_t e = S + 3 * p.stride + p.flen + 4 - sn;
        dma_item(slot, sn, lane, (uint32_t)(e < (uint64_t)kDmaItemBytes ? e : (uint64_t)kDmaItemBytes));
    };

    uint64_t it = D.first();
    if (it != kEnd) dma_of(it);
    while (it != kEnd) {   // wave-uniform
        const uint64_t f = 4 * it + (uint64_t)g;
        const uint64_t S = item_start(it), src = slot_src(S);
        __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0): this wave's slot DMA has landed
        // a frame past the batch's end (last item) works on the item's first frame: nothing outside the
        // slot is read, and nothing is stored for it
        const uint64_t goff = f < p.n ? (uint64_t)g * p.stride : 0ull;
        const int64_t x = (int64_t)(S - src + goff) + rel;   // window start within the slot
        const uint32_t r = (uint32_t)x & 3u;
        const uint32_t *wp = reinterpret_cast<const uint32_t *>(slot + (x & ~3ll));
        uint32_t d[kChunkWords + 1];
#pragma unroll
        for (int q = 0; q < kChunkWords; q++) d[q] = wp[q];
        {   // the 25th dword matters only when r != 0; clamped so the slot is never read past its end
            const uint64_t a24 = (uint64_t)(wp + kChunkWords), lim = (uint64_t)(slot + kDmaItemBytes - 4);
            d[kChunkWords] = *reinterpret_cast<const uint32_t *>(a24 < lim ? a24 : lim);
        }
        // the frame's first 128 bytes: dwords c and c + 16 from floor4(frame start) in the slot
        Frame fr;
        fr.start = S + goff;   // slots start at 16-B pieces: same low address bits
        fr.len = p.flen;
        fr.m = 1;
        Chunk ch;
        {
            const uint32_t hb = (uint32_t)(S - src + goff) & ~3u;
            const uint32_t *hp = reinterpret_cast<const uint32_t *>(slot + hb);
            ch.h0 = hp[c];
            ch.h1 = hp[c + 16];
        }
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA
        const uint64_t nxt = D.next(it);
        if (nxt != kEnd) dma_of(nxt);

        const THdr H = decode(fr, ch, c, tp.flags);
        uint32_t w[kChunkWords];
#pragma unroll
        for (int i = 0; i < kChunkWords; i++) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], r);
#pragma unroll
        for (int i = 0; i < kSingleMaskWords; i++) {   // zc <= 28: the first 7 words at most
            int t = zc - 4 * i;
            t = t < 0 ? 0 : (t > 4 ? 4 : t);
            w[i] &= (uint32_t)(0xFFFFFFFFull << (8 * t));
        }
        uint64_t tot = 0, tail = 0;
#pragma unroll
        for (int i = 0; i < kChunkWords; i += 2) tot += (uint64_t)w[i] + w[i + 1];
        {
            const int dl = H.cl - rel;
            const int dt = !H.ps ? kChunkBytes + 4 : (dl < -4 ? -4 : (dl > kChunkBytes + 4 ? kChunkBytes + 4 : dl));
#pragma unroll
            for (int blk = 0; blk < 4; blk++) {
                if (__any(dt < 24 * (blk + 1))) {
#pragma unroll
                    for (int i = 6 * blk; i < 6 * blk + 6; i++) tail += clear_low_bits(w[i], 8 * (dt - 4 * i));
                }
            }
        }
        const Seal z = seal_of(H, tot, tail, p.flen & 1u, fr.start & 1ull);
        const bool st = f < p.n;
        const uint32_t v = H.bits | (FCSW ? kFcsSet : 0u);
        store_sums(tp, st, c, f, fr.start, H, z, v);
        const uint64_t mb = __ballot(st && c == kGroup - 1 && (v & p.bad_mask) != 0u);
        if (mb != 0 && lane == 0) *wave_bad<kDmaBad>(lds) += (uint64_t)__popcll(mb);
        uint32_t crc = 0u;
        if (FCSW) {
            // the IP field's place is a loop invariant: kept opaque, or its 48 word compares are
            // hoisted into scalar register pairs that then spill
            int bip = 24 - rel;
            asm volatile("" : "+v"(bip));
            xor_field(w, bip, z.dip);
            xor_field(w, H.ql4 ? H.ql4 - rel : kNoField, z.dl4);
            // the lookups' per-lane bases and selectors (rxv_dma_kernel's), lane table base and INV start,
            // formed here from an opaque lane number: as loop invariants they would hold ten registers
            // through the sums
            uint32_t ln = (uint32_t)lane;
            asm volatile("" : "+v"(ln));
            const uint32_t h = (ln >> 3) & 3u, r4 = (ln & 7u) * 4u;
            const uint32_t lanebase = kDmaHole + (ln & 31u) * 4u;
            const uint32_t x0 = (ln & 15u) == (uint32_t)(kGroup - 1)   // the front lane's INV start
                                    ? lds_rd(lds, dma_hole(kDmaInvHole + (uint32_t)zc / 32u) + (uint32_t)(zc % 32) * 4u)
                                    : 0u;
            const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
            const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                                     0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
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
            crc = ~row_xor(lane_shift_dma(lds, mv, lanebase));
        }
        store_fcs<FCSW>(tp, st, c, f, fr.start, p.flen, crc);
        it = nxt;
    }
    if (p.bad != nullptr && lane == 0) {
        const uint64_t b = *wave_bad<kDmaBad>(lds);
        if (b) atomicAdd(p.bad, (unsigned long long)b);
    }
}

// The one routing decision (launch_txs launches what it returns; the engine leases a work counter
// exactly when it returns kDma).
Route route(bool var, const TParams &tp, uint64_t dma_min) {
    const RParams &p = tp.r;
    if (!p.n) return Route::kNone;
    if (var || p.n <= dma_min) return Route::kGeneral;
    if ((tp.flags & kFlagFcs) && p.stride < (uint64_t)p.flen + 4) return Route::kGeneral;
    fcs::KParams k{};
    k.stride = p.stride;
    k.flen = p.flen;
    k.fseg = 1;
    k.lo4 = p.lo4;
    k.hi4 = p.hi4;
    return fcs::fixed_dma(k) ? Route::kDma : Route::kGeneral;
}

namespace {
std::atomic<int> g_last_route{(int)Route::kNone};
}
Route last_launch() { return (Route)g_last_route.load(std::memory_order_relaxed); }

hipError_t launch_txs(bool var, const TParams &tp, int cus, uint64_t dma_min, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    const RParams &p = tp.r;
    const bool fcsw = (tp.flags & kFlagFcs) != 0;
    const Route rt = route(var, tp, dma_min);
    if (rt == Route::kNone) return hipSuccess;
    g_last_route.store((int)rt, std::memory_order_relaxed);
    if (rt == Route::kDma) {
        if (!p.ctr) return hipErrorInvalidValue;
        const uint64_t items = (p.n + 3) / 4, wantd = (items + kDmaThreads / 64 - 1) / (kDmaThreads / 64);
        const int gd = (int)(wantd < (uint64_t)cus ? wantd : (uint64_t)cus);
        if (fcsw) hipLaunchKernelGGL((txs_dma_kernel<true>), dim3(gd), dim3(kDmaThreads), 0, st, tp);
        else hipLaunchKernelGGL((txs_dma_kernel<false>), dim3(gd), dim3(kDmaThreads), 0, st, tp);
        return hipGetLastError();
    }
    const bool tiny = p.hi4 - p.lo4 < 2 * (uint64_t)kChunkBytes;
    // one workgroup per CU, persistent over the frames (a quarter-wave per frame)
    const uint64_t slots = kThreads / kGroup, want = (p.n + slots - 1) / slots;
    const int grid = (int)(want < (uint64_t)cus ? want : (uint64_t)cus);
#define TXS_GO(V, T, S) hipLaunchKernelGGL((txs_kernel<V, T, S, kThreads>), dim3(grid), dim3(kThreads), 0, st, tp)
    if (var) {
        if (fcsw) { if (tiny) TXS_GO(true, true, true); else TXS_GO(true, true, false); }
        else { if (tiny) TXS_GO(true, false, true); else TXS_GO(true, false, false); }
    } else {
        if (fcsw) { if (tiny) TXS_GO(false, true, true); else TXS_GO(false, true, false); }
        else { if (tiny) TXS_GO(false, false, true); else TXS_GO(false, false, false); }
    }
#undef TXS_GO
    return hipGetLastError();
}

}  // namespace txs
