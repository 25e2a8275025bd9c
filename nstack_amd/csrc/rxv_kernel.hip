// rxv_kernel.hip — one-pass RX validation for gfx950: FCS residue, IPv4 header and L4 checksums
// of every frame of a batch from ONE read of its bytes (include/nstack_rxv.h has the verdict rules
// and the reference lines they restate).
//
// Work decomposition: the generic FCS kernel's (fcs_kernel.hip). A QUARTER-WAVE (16 lanes) per
// frame; lane j owns the 96-byte chunk that ends 96 j bytes before the frame end (6 dwordx4 + 1
// dword from a 4-byte aligned address, re-aligned to the frame end with v_alignbyte_b32, bytes in
// front of the frame start zeroed); longer frames are walked in 1536-byte segments. The loads of
// the next chunk are in flight while the current one is worked on.
//   * CRC (RXV_F_TRAILER only): the per-lane slice-by-4 recurrence over the 24 words, joined across
//     the lanes with the per-lane shift tables (fcs_crc.hpp; the FCS engine's table blob in LDS).
//   * Sums: the same 24 re-aligned words are added as whole dwords into a 64-bit register (2^16 == 1
//     mod 0xffff, inet_kernel.hip). The frame total needs no mask of its own (the CRC's front mask
//     serves); the bytes behind the L4 segment (padding, FCS trailer: frame bytes from 14 + ip_len)
//     are summed a second time under a mask, only in the 6-word blocks some lane of the wave has
//     such bytes in (the last one or two of the end lane for real traffic).
//   * Header: lane l of the frame also loads dwords l and l + 16 of the frame's first 128 bytes
//     (an L1/L2 hit on lines the chunk loads read anyway), issued with the chunk loads, one item
//     ahead. The fields (frame bytes 12..33, the UDP checksum field) come from them by
//     ds_bpermute, so the cuts are known before the frame's first chunk is summed; the sums of
//     frame bytes [14, 14 + hlen) (the IP header) and [0, 14 + hlen) from the same two dwords,
//     masked per lane.
//   * L4 sum = total - [0, 14 + hlen) - [14 + ip_len, F) in one's-complement arithmetic. The three
//     parts are sums of 16-bit words on different grids (the frame end's, memory's); a sum on a
//     grid that pairs the region's bytes the other way round is the byte-swapped sum
//     (P = swap16(fold(M)), inet_kernel.hip), and the header and segment both start at an even
//     frame byte, so each part is swapped to the frame start's grid before they are combined.
//   * Every check is "the reference function returns non-zero": ip_checksum and tcp_checksum start
//     at 0xffff and keep the running sum in 1..0xffff, udp_checksum adds the non-zero protocol
//     word, so the folded total is never 0 and the function returns 0 exactly when it is 0xffff.
//     The pseudo headers are built from the header's own address words (pseudo_sd's formulas,
//     inet_kernel.hip, the mode chosen per frame by ip_proto).
// The verdict is assembled by every lane of the frame (row-uniform); the frame's front lane (15)
// stores it. Frames with verdict & bad_mask are counted per wave in LDS and added to *bad once at
// exit. rxv_dma_kernel (below) is the same arithmetic on fcs_dma_kernel's load form for fixed
// strides of 1496..1524-B frames; rxv::route decides between the two.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "frame_walk.hpp"
#include "rxv_launch.hpp"

namespace rxv {

// What a frame's header decided before its first chunk is summed (uniform over the frame's lanes).
struct Hdr {
    uint32_t bits;    // verdict bits that need no sum
    uint32_t ps;      // L4: accumulator start plus pseudo header; 0 = no L4 checksum to verify
    int cl;           // frame position of the first byte behind the L4 segment (tail mask)
    uint32_t sums;    // this lane's header_sums
};

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
                h.ps = ones::l4_start(proto, src, dst, iplen - hlen, ufield, kL4Short, h.bits);   // rule 8
                if (h.ps) {
                    h.bits |= kL4Checked;
                    h.cl = 14 + (int)iplen;
                }
            }
        }
    }
    h.sums = header_sums(ch, j, r, che);
    return h;
}

// The verdict's checksum bits, from the reduced sums (row-uniform): every check is "the reference
// function returns non-zero".
__device__ __forceinline__ uint32_t sum_verdict(uint32_t v, const Hdr &H, uint64_t tot, uint64_t tail, bool odd_len,
                                                bool odd_start) {
    const Sums z = reduce_sums(tot, tail, H.sums, odd_len, odd_start);
    if ((v & (kIpv4 | kIpBadHdr)) == kIpv4 && fold64(0xffffull + z.hdr_s) != 0xffffu) v |= kIpBadCsum;
    // the common case, said so: without the hint both checks were laid out of line in rxv_kernel (a
    // jump out and back per frame; IMIX with the CRC 34.17 against 33.44 ms, with it 33.30 against
    // 33.92). rxv_dma_kernel shares the function; its rows measure the same with the hint as before.
    if (__builtin_expect(H.ps != 0u, 1)) {
        const uint64_t l4 = (uint64_t)H.ps + z.tot_s + (0xffffu - z.head_s) + (0xffffu - z.tail_s);
        if (fold64(l4) != 0xffffu) v |= kL4BadCsum;
    }
    return v;
}

template <bool VAR, bool TRAILER, bool TINY, int NT>
__global__ __launch_bounds__(NT, 1) void rxv_kernel(RParams p) {
    // without the CRC only the per-wave bad counters live in LDS
    constexpr uint32_t kBad = TRAILER ? fcs::kLdsBad : 0u;
    __shared__ __attribute__((aligned(16))) uint8_t lds[TRAILER ? fcs::kLdsBytes : 16 * 8];
    if (TRAILER) fcs::stage_tables<NT>(tables_of(p.blob), lds);
    fcs::init_bad<kBad>(lds);
    const int lane = threadIdx.x & 63, j = lane & (kGroup - 1);
    uint32_t tb0, tb1;
    fcs::table_bases(lane, tb0, tb1);
    const uint32_t lanebase = fcs::kLdsLane | ((uint32_t)(lane & 31) * 4u);
    const uint64_t Q = (uint64_t)gridDim.x * (NT / kGroup);   // frame slots in the grid

    // per-frame state, carried over the frame's segments
    uint32_t s = 0;            // CRC register
    uint64_t tot = 0, tail = 0;
    Hdr H{0u, 0u, 0, 0u};

    auto process = [&](const Pos &c, const Chunk &ch) {
        uint32_t w[kChunkWords];
        chunk_words<TINY>(ch, w);
        const bool first = c.k == 0;
        if (__any(first)) {   // a frame's first chunk: its header fields
            const Hdr hn = decode<TRAILER>(c.fr, ch, j);
            if (first) {
                H = hn;
                if (!c.act) H.bits = H.ps = 0u;
                tot = tail = 0;
            }
        }
        if (first) front_mask(w, ch.zr, (int)p.zmax);
        add_sums(w, rel_of(c.fr.len, c.fr.m, c.k, j), H.cl, H.ps, tot, tail);
        if (TRAILER) s = crc_step(lds, s, w, first, ch.zr, tb0, tb1);
        // ---- the frame's last chunk: join the lanes, assemble the verdict ----
        const bool last = c.act && c.k + 1 == c.fr.m;
        if (__any(last)) {
            uint32_t v = H.bits;
            if (TRAILER) {
                const uint32_t x = crc_join(lds, s, last, lanebase);
                if ((c.fr.len ? ~x : 0u) != fcs::kResidue) v |= kFcsBad;
            }
            v = sum_verdict(v, H, tot, tail, c.fr.len & 1u, c.fr.start & 1ull);
            const bool st = last && j == 15;
            if (st) p.verdict[c.f] = v;
            count_bad(fcs::wave_bad<kBad>(lds), lane, st && (v & p.bad_mask) != 0u);
        }
    };

    two_in_flight<Chunk>(
        first_pos<VAR>(p, (uint64_t)blockIdx.x * (NT / kGroup) + threadIdx.x / kGroup),
        [&](const Pos &c) { return next_pos<VAR>(p, c, Q); },
        [&](const Pos &c, Chunk &ch) { issue<TINY>(p, c, j, ch); }, process);
    flush_bad(fcs::wave_bad<kBad>(lds), lane, p.bad);
}

// ---------------------------------------------------------------------------------------------
// Fixed-stride batches through LDS (rxv_dma_kernel): fcs_dma_kernel's load form and CRC. A wave
// item is four consecutive frames of 1496..1524 B that fit a 6 KiB slot (fcs::fixed_dma); the
// item arrives in the wave's slot by six global_load_lds rows (whole 16-B pieces inside
// [floor16(lo4), ceil16(hi4))), the next item's DMA is in flight while the current one is worked on,
// items come from the work dispenser, 16 waves per CU. Quarter g of the wave takes frame g: lane c
// reads its window [E - e_c - 96, E - e_c) from the slot (e_c = dma_end_off(c); the front lane's
// leading bytes and the overlap word of lanes 3, 7, 11 masked, so every frame byte is in exactly
// one lane's words), and its header dwords c and c + 16 from the frame's start in the slot
// (frame_walk.hpp's DmaSlots and dma_window). The CRC is fcs_dma_kernel's (two chains on the
// 8-replica slice tables, merge, lane shift, row XOR); sums, header decode and verdict are
// rxv_kernel's, from the same window registers, with the geometry a loop invariant (fixed length).
// The frame's front lane stores the verdict.
// ---------------------------------------------------------------------------------------------
template <bool TRAILER>
__global__ __launch_bounds__(kDmaThreads, 1) void rxv_dma_kernel(RParams p) {
    using namespace fcs;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDmaRing + (kDmaThreads / 64) * kDmaItemBytes];
    const int tid = threadIdx.x;
    if (TRAILER) stage_dma_tables<kDmaThreads>(tables_of(p.blob), lds, tid);
    init_bad<kDmaBad>(lds);
    __syncthreads();

    const int lane = tid & 63;
    const int c = lane & (kGroup - 1);     // chunk index back from the frame end
    const int g = lane >> 4;               // frame of the item
    const DmaSlots G(p, lds, __builtin_amdgcn_readfirstlane(tid >> 6), lane);

    // loop invariants: the lookups' lane constants, the window's place in the frame, leading bytes
    // to mask, INV start
    const DmaLane L = dma_lane((uint32_t)lane);
    const int rel = (int)p.flen - (int)dma_end_off(c) - kChunkBytes;   // frame position of the window's first byte (>= -28)
    const int zc = (c == kGroup - 1) ? (int)(kDmaCover - p.flen) : (dma_short_lane(c) ? 4 : 0);
    const uint32_t x0 = TRAILER ? dma_inv_start(lds, (uint32_t)lane, zc) : 0u;

    constexpr uint64_t kEnd = Dispenser::kEnd;
    Dispenser D = G.dispenser();
    uint64_t it = D.first();
    if (it != kEnd) G.dma_of(it);
    while (it != kEnd) {   // wave-uniform
        uint32_t d[kChunkWords + 1], r;
        Frame fr;
        Chunk ch;
        const uint64_t f = dma_window(G, it, g, c, rel, d, r, fr, ch);
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the slot is free for the next DMA
        const uint64_t nxt = D.next(it);
        if (nxt != kEnd) G.dma_of(nxt);

        const Hdr H = decode<TRAILER>(fr, ch, c);
        uint32_t w[kChunkWords];
        align_words(d, r, w);
        front_mask(w, zc, 4 * kSingleMaskWords);   // zc <= 28: the first 7 words at most
        uint64_t tot = 0, tail = 0;
        add_sums(w, rel, H.cl, H.ps, tot, tail);
        uint32_t v = H.bits;
        if (TRAILER && ~row_xor(dma_chunk_crc(lds, w, x0, L.B, L.SEL, L.lanebase)) != kResidue) v |= kFcsBad;
        v = sum_verdict(v, H, tot, tail, p.flen & 1u, fr.start & 1ull);
        const bool st = c == kGroup - 1 && f < p.n;
        if (st) p.verdict[f] = v;
        count_bad(wave_bad<kDmaBad>(lds), lane, st && (v & p.bad_mask) != 0u);
        it = nxt;
    }
    flush_bad(wave_bad<kDmaBad>(lds), lane, p.bad);
}

// The one routing decision (launch_rxv launches what it returns; the engine leases a work counter
// exactly when it returns kDma).
Route route(bool var, const RParams &p, uint64_t dma_min) { return dma_band_route(var, p, dma_min); }

namespace {
std::atomic<int> g_last_route{(int)Route::kNone};
}
Route last_launch() { return (Route)g_last_route.load(std::memory_order_relaxed); }

hipError_t launch_rxv(bool var, bool trailer, const RParams &p, int cus, uint64_t dma_min, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    const Route rt = route(var, p, dma_min);
    if (rt == Route::kNone) return hipSuccess;
    g_last_route.store((int)rt, std::memory_order_relaxed);
    if (rt == Route::kDma) {
        if (!p.ctr) return hipErrorInvalidValue;
        const int gd = dma_grid(p.n, cus);
        if (trailer) hipLaunchKernelGGL((rxv_dma_kernel<true>), dim3(gd), dim3(kDmaThreads), 0, st, p);
        else hipLaunchKernelGGL((rxv_dma_kernel<false>), dim3(gd), dim3(kDmaThreads), 0, st, p);
        return hipGetLastError();
    }
    FRAME_WALK_LAUNCH(rxv_kernel, var, trailer, walk_tiny(p), walk_grid(p.n, cus), st, p);
    return hipGetLastError();
}

}  // namespace rxv
