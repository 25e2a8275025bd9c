// txs_kernel.hip — one-pass TX sealing for gfx950: the IPv4 header checksum, the TCP / UDP / ICMP
// checksum and the FCS of every frame of a batch, computed from ONE read of its bytes and stored in
// place (include/nstack_txs.h has the rules and the reference lines they restate). The mirror image
// of rxv_kernel.hip, whose frame walk, loads, sums and CRC forms it shares (frame_walk.hpp,
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

#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "frame_walk.hpp"
#include "txs_launch.hpp"

namespace txs {

using fcs::kChunkBytes;
using fcs::kChunkWords;
using fcs::kGroup;
using rxv::Chunk;
using rxv::fold64;
using rxv::Frame;
using rxv::kNoField;
using rxv::Pos;
using rxv::row_get;
using rxv::RParams;
using rxv::swap16;
using rxv::xor_field;

// What a frame's header decided before its first chunk is summed (uniform over the frame's lanes).
struct THdr {
    uint32_t bits;    // status bits that need no sum
    uint32_t ps;      // L4: accumulator start plus pseudo header; 0 = no L4 sum
    uint32_t old;     // the fields' old content, words of the frame start's grid: IP | L4 << 16
    uint32_t sums;    // this lane's rxv::header_sums (both with the old field content)
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
    h.sums = rxv::header_sums(ch, j, r, h.che);
    return h;
}

// The values to write, from the reduced sums (row-uniform).
struct Seal {
    uint32_t ip, l4;     // the uint16 values as stored (low byte at the lower address)
    uint32_t dip, dl4;   // new ^ old; 0 where nothing is written
};

__device__ __forceinline__ Seal seal_of(const THdr &H, uint64_t tot, uint64_t tail, bool odd_len, bool odd_start) {
    Seal z{0u, 0u, 0u, 0u};
    const rxv::Sums q = rxv::reduce_sums(tot, tail, H.sums, odd_len, odd_start);
    const uint32_t oip = H.old & 0xffffu, ol4 = H.old >> 16;
    if (H.che) {
        // three 16-bit terms: summed in 32 bits. Behind rxv::reduce_sums the compiler no longer proves that
        // itself as it did before, and the 64-bit sum it then forms shows in the variable-length rows
        // (IMIX without FCS 26.23 and 26.19 against 26.13 and 26.12 ms with this form; before 26.21)
        z.ip = ~fold64(0xffffu + q.hdr_s + (0xffffu - oip)) & 0xffffu;
        z.dip = z.ip ^ oip;
    }
    if (H.ql4) {
        if (H.ps) {
            const uint64_t l4 = (uint64_t)H.ps + q.tot_s + (0xffffu - q.head_s) + (0xffffu - q.tail_s) + (0xffffu - ol4);
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

template <bool VAR, bool FCSW, bool TINY, int NT>
__global__ __launch_bounds__(NT, 1) void txs_kernel(TParams tp) {
    const RParams &p = tp.r;
    // without the CRC only the per-wave counters live in LDS
    constexpr uint32_t kBad = FCSW ? fcs::kLdsBad : 0u;
    __shared__ __attribute__((aligned(16))) uint8_t lds[FCSW ? fcs::kLdsBytes : 16 * 8];
    if (FCSW) fcs::stage_tables<NT>(rxv::tables_of(p.blob), lds);
    fcs::init_bad<kBad>(lds);
    const int lane = threadIdx.x & 63, j = lane & (kGroup - 1);
    uint32_t tb0, tb1;
    fcs::table_bases(lane, tb0, tb1);
    const uint32_t lanebase = fcs::kLdsLane | ((uint32_t)(lane & 31) * 4u);
    const uint64_t Q = (uint64_t)gridDim.x * (NT / kGroup);   // frame slots in the grid

    // per-frame state, carried over the frame's segments
    uint32_t s = 0;            // CRC register
    uint64_t tot = 0, tail = 0;
    THdr H{0u, 0u, 0u, 0u, 0, 0, 0};

    auto process = [&](const Pos &c, const Chunk &ch) {
        uint32_t w[kChunkWords];
        rxv::chunk_words<TINY>(ch, w);
        const bool first = c.k == 0;
        if (__any(first)) {   // a frame's first chunk: its header fields
            const THdr hn = decode(c.fr, ch, j, tp.flags);
            if (first) {
                H = hn;
                if (!c.act) H = THdr{0u, 0u, 0u, 0u, 0, 0, 0};
                tot = tail = 0;
            }
        }
        if (first) rxv::front_mask(w, ch.zr, (int)p.zmax);
        rxv::add_sums(w, rxv::rel_of(c.fr.len, c.fr.m, c.k, j), H.cl, H.ps, tot, tail);
        // ---- the frame's last chunk: the values; a single-segment frame is patched in its registers ----
        const bool last = c.act && c.k + 1 == c.fr.m;
        Seal z{0u, 0u, 0u, 0u};
        if (__any(last)) {
            z = seal_of(H, tot, tail, c.fr.len & 1u, c.fr.start & 1ull);
            if (FCSW) {
                const bool one = last && first;
                // frame position of the chunk's first byte; used for a single segment only (<= 1536 - 96)
                const int rel = (int)rxv::rel_of(c.fr.len, 1u, 0u, j);
                xor_field(w, one ? 24 - rel : kNoField, z.dip);
                xor_field(w, one && H.ql4 ? H.ql4 - rel : kNoField, z.dl4);
            }
        }
        if (FCSW) s = rxv::crc_step(lds, s, w, first, ch.zr, tb0, tb1);
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
                    const int rel = (int)rxv::rel_of(F, 1u, 0u, (int)ci);   // chunk ci counted from the frame end
                    uint32_t dw[kChunkWords];
#pragma unroll
                    for (int i = 0; i < kChunkWords; i++) dw[i] = 0u;
                    xor_field(dw, own ? 24 - rel : kNoField, z.dip);
                    xor_field(dw, own && H.ql4 ? H.ql4 - rel : kNoField, z.dl4);
                    uint32_t rd = fcs::chunk_crc(lds, dw, 0u, tb0, tb1);
                    const uint32_t cnt = own ? ci >> 4 : 0u;   // segments behind the chunk's
                    for (uint32_t t = 0; __any(t < cnt); t++) {
                        const uint32_t nx = fcs::uniform_shift<fcs::kLdsJump>(lds, rd, 0u);
                        rd = t < cnt ? nx : rd;
                    }
                    s ^= own ? rd : 0u;
                }
                const uint32_t x = rxv::crc_join(lds, s, last, lanebase);
                crc = c.fr.len ? ~x : 0u;
                v |= kFcsSet;
            }
            store_sums(tp, last, j, c.f, c.fr.start, H, z, v);
            store_fcs<FCSW>(tp, last, j, c.f, c.fr.start, c.fr.len, crc);
            rxv::count_bad(fcs::wave_bad<kBad>(lds), lane, last && j == 15 && (v & p.bad_mask) != 0u);
        }
    };

    // rxv::next_pos, first_pos and two_in_flight written out here, the one piece of the walk this
    // kernel does not share: through them the variable-length rows ran 0.9 % slower than before
    // (IMIX without FCS 26.43 against 26.19 ms), written out they run as before
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
    Pos A, B;
    A.f = (uint64_t)blockIdx.x * (NT / kGroup) + threadIdx.x / kGroup;
    A.k = 0;
    A.act = A.f < p.n;
    A.fr = A.act ? rxv::frame_of<VAR>(p, A.f) : Frame{0, 0, 1};
    Chunk CA, CB;
    rxv::issue<TINY>(p, A, j, CA);
    while (__any(A.act)) {
        B = next(A);
        rxv::issue<TINY>(p, B, j, CB);
        process(A, CA);
        if (!__any(B.act)) break;
        A = next(B);
        rxv::issue<TINY>(p, A, j, CA);
        process(B, CB);
    }
    rxv::flush_bad(fcs::wave_bad<kBad>(lds), lane, p.bad);
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
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDmaRing + (kDmaThreads / 64) * kDmaItemBytes];
    const int tid = threadIdx.x;
    if (FCSW) stage_dma_tables<kDmaThreads>(rxv::tables_of(p.blob), lds, tid);
    init_bad<kDmaBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const int c = lane & (kGroup - 1);     // chunk index back from the frame end
    const int g = lane >> 4;               // frame of the item
    const rxv::DmaSlots G(p, lds, __builtin_amdgcn_readfirstlane(tid >> 6), lane);

    // loop invariants: the window's place in the frame, leading bytes to mask
    const int rel = (int)p.flen - (int)dma_end_off(c) - kChunkBytes;   // frame position of the window's first byte (>= -28)
    const int zc = (c == kGroup - 1) ? (int)(kDmaCover - p.flen) : (dma_short_lane(c) ? 4 : 0);

    constexpr uint64_t kEnd = Dispenser::kEnd;
    Dispenser D = G.dispenser();
    uint64_t it = D.first();
    if (it != kEnd) G.dma_of(it);
    while (it != kEnd) {   // wave-uniform
        uint32_t d[kChunkWords + 1], r;
        Frame fr;
        Chunk ch;
        const uint64_t f = rxv::dma_window(G, it, g, c, rel, d, r, fr, ch);   // past the batch's end: nothing is stored
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA
        const uint64_t nxt = D.next(it);
        if (nxt != kEnd) G.dma_of(nxt);

        const THdr H = decode(fr, ch, c, tp.flags);
        uint32_t w[kChunkWords];
        rxv::align_words(d, r, w);
        rxv::front_mask(w, zc, 4 * kSingleMaskWords);   // zc <= 28: the first 7 words at most
        uint64_t tot = 0, tail = 0;
        rxv::add_sums(w, rel, H.cl, H.ps, tot, tail);
        const Seal z = seal_of(H, tot, tail, p.flen & 1u, fr.start & 1ull);
        const bool st = f < p.n;
        const uint32_t v = H.bits | (FCSW ? kFcsSet : 0u);
        store_sums(tp, st, c, f, fr.start, H, z, v);
        rxv::count_bad(wave_bad<kDmaBad>(lds), lane, st && c == kGroup - 1 && (v & p.bad_mask) != 0u);
        uint32_t crc = 0u;
        if (FCSW) {
            // the IP field's place is a loop invariant: kept opaque, or its 48 word compares are
            // hoisted into scalar register pairs that then spill
            int bip = 24 - rel;
            asm volatile("" : "+v"(bip));
            xor_field(w, bip, z.dip);
            xor_field(w, H.ql4 ? H.ql4 - rel : kNoField, z.dl4);
            // the lookups' lane constants and the INV start (rxv_dma_kernel's), formed here from an
            // opaque lane number: as loop invariants they would hold ten registers through the sums
            uint32_t ln = (uint32_t)lane;
            asm volatile("" : "+v"(ln));
            const uint32_t x0 = dma_inv_start(lds, ln, zc);
            const DmaLane L = dma_lane(ln);
            crc = ~row_xor(dma_chunk_crc(lds, w, x0, L.B, L.SEL, L.lanebase));
        }
        store_fcs<FCSW>(tp, st, c, f, fr.start, p.flen, crc);
        it = nxt;
    }
    rxv::flush_bad(wave_bad<kDmaBad>(lds), lane, p.bad);
}

// The one routing decision (launch_txs launches what it returns; the engine leases a work counter
// exactly when it returns kDma).
Route route(bool var, const TParams &tp, uint64_t dma_min) {
    const RParams &p = tp.r;
    if (p.n && (tp.flags & kFlagFcs) && p.stride < (uint64_t)p.flen + 4) return Route::kGeneral;   // no FCS place
    return rxv::dma_band_route(var, p, dma_min);
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
        const int gd = rxv::dma_grid(p.n, cus);
        if (fcsw) hipLaunchKernelGGL((txs_dma_kernel<true>), dim3(gd), dim3(kDmaThreads), 0, st, tp);
        else hipLaunchKernelGGL((txs_dma_kernel<false>), dim3(gd), dim3(kDmaThreads), 0, st, tp);
        return hipGetLastError();
    }
    FRAME_WALK_LAUNCH(txs_kernel, var, fcsw, rxv::walk_tiny(p), rxv::walk_grid(p.n, cus), st, tp);
    return hipGetLastError();
}

}  // namespace txs
