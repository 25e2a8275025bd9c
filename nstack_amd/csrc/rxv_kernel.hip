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

#include "dispenser.hpp"
#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "rxv_launch.hpp"
#include "rxv_parts.hpp"

namespace rxv {

template <bool VAR, bool TRAILER, bool TINY, int NT>
__global__ __launch_bounds__(NT, 1) void rxv_kernel(RParams p) {
    // without the CRC only the per-wave bad counters live in LDS
    constexpr uint32_t kBad = TRAILER ? fcs::kLdsBad : 0u;
    __shared__ __attribute__((aligned(16))) uint8_t lds[TRAILER ? fcs::kLdsBytes : 16 * 8];
    if (TRAILER) {
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
        if (n.act && n.k == 0) n.fr = frame_of<VAR>(p, n.f);
        return n;
    };

    // per-frame state, carried over the frame's segments
    uint32_t s = 0;            // CRC register
    uint64_t tot = 0, tail = 0;
    Hdr H{0u, 0u, 0, 0u};

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
            const Hdr hn = decode<TRAILER>(c.fr, ch, j);
            if (first) {
                H = hn;
                if (!c.act) H.bits = H.ps = 0u;
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
        // ---- sums: every word into the total; words holding bytes from cl on also into the tail ----
        {
            uint64_t a = 0;
#pragma unroll
            for (int i = 0; i < kChunkWords; i += 2) a += (uint64_t)w[i] + w[i + 1];
            tot += a;
            // frame position of this chunk's first byte, and cl relative to it (clamped: the masks
            // clamp again, this keeps the arithmetic inside an int)
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
        // ---- CRC: two independent 12-word chains, merged with A_48 (fcs_kernel.hip) ----
        if (TRAILER) {
            uint32_t x0 = 0;
            if (first) {
                const int zi = ch.zr < 0 ? 0 : (ch.zr > kChunkBytes - 1 ? kChunkBytes - 1 : ch.zr);
                const uint32_t iv = fcs::lds_rd(lds, fcs::kLdsInv + 4u * (uint32_t)zi);
                x0 = (ch.zr >= 0 && ch.zr < kChunkBytes) ? iv : 0u;
            }
            uint32_t xa = x0 ^ w[0], xb = w[12];
#pragma unroll
            for (int i = 0; i < 12; i++) {
                xa = fcs::step4(lds, xa, i < 11 ? w[i + 1] : 0u, tb0, tb1);
                xb = fcs::step4(lds, xb, i < 11 ? w[13 + i] : 0u, tb0, tb1);
            }
            const uint32_t rr = fcs::uniform_shift<fcs::kLdsH48>(lds, xa, xb);
            s = first ? rr : fcs::uniform_shift<fcs::kLdsJump>(lds, s, rr);
        }
        // ---- the frame's last chunk: join the lanes, assemble the verdict ----
        const bool last = c.act && c.k + 1 == c.fr.m;
        if (__any(last)) {
            uint32_t v = H.bits;
            if (TRAILER) {
                uint32_t x = last ? fcs::lane_shift(lds, s, lanebase) : 0u;
                x = fcs::row_xor(x);
                if ((c.fr.len ? ~x : 0u) != fcs::kResidue) v |= kFcsBad;
            }
            const uint32_t te = fold64(row_sum(fold64(tot))), ta = fold64(row_sum(fold64(tail)));
            const uint32_t hm = fold64(row_sum(H.sums & 0xffffu)), h0 = fold64(row_sum(H.sums >> 16));
            // to the frame start's word grid: the end grid differs for an odd length, memory's for an odd start
            const bool oe = c.fr.len & 1u, om = c.fr.start & 1ull;
            const uint32_t tot_s = oe ? swap16(te) : te, tail_s = oe ? swap16(ta) : ta;
            const uint32_t hdr_s = om ? swap16(hm) : hm, head_s = om ? swap16(h0) : h0;
            if ((v & (kIpv4 | kIpBadHdr)) == kIpv4 && fold64(0xffffull + hdr_s) != 0xffffu) v |= kIpBadCsum;
            if (H.ps) {
                const uint64_t l4 = (uint64_t)H.ps + tot_s + (0xffffu - head_s) + (0xffffu - tail_s);
                if (fold64(l4) != 0xffffu) v |= kL4BadCsum;
            }
            const bool st = last && j == 15;
            if (st) p.verdict[c.f] = v;
            const uint64_t mb = __ballot(st && (v & p.bad_mask) != 0u);
            if (mb != 0 && lane == 0) *fcs::wave_bad<kBad>(lds) += (uint64_t)__popcll(mb);
        }
    };

    Pos A, B;
    A.f = (uint64_t)blockIdx.x * (NT / kGroup) + threadIdx.x / kGroup;
    A.k = 0;
    A.act = A.f < p.n;
    A.fr = A.act ? frame_of<VAR>(p, A.f) : Frame{0, 0, 1};
    Chunk CA, CB;
    issue<TINY>(p, A, j, CA);
    // two items in flight per lane: process one while the other's loads are outstanding
    while (__any(A.act)) {
        B = next(A);
        issue<TINY>(p, B, j, CB);
        process(A, CA);
        if (!__any(B.act)) break;
        A = next(B);
        issue<TINY>(p, A, j, CA);
        process(B, CB);
    }
    if (p.bad != nullptr && lane == 0) {
        const uint64_t b = *fcs::wave_bad<kBad>(lds);
        if (b) atomicAdd(p.bad, (unsigned long long)b);
    }
}

// ---------------------------------------------------------------------------------------------
// Fixed-stride batches through LDS (rxv_dma_kernel): fcs_dma_kernel's load form and CRC. A wave
// item is four consecutive frames of 1496..1524 B that fit a 6 KiB slot (fcs::fixed_dma); the
// item arrives in the wave's slot by six global_load_lds rows (whole 16-B pieces inside
// [floor16(lo4), ceil16(hi4))), the next item's DMA is in flight while the current one is worked on,
// items come from the work dispenser, 16 waves per CU. Quarter g of the wave takes frame g: lane c
// reads its window [E - e_c - 96, E - e_c) from the slot (e_c = dma_end_off(c); the front lane's
// leading bytes and the overlap word of lanes 3, 7, 11 masked, so every frame byte is in exactly
// one lane's words), and its header dwords c and c + 16 from the frame's start in the slot. The
// CRC is fcs_dma_kernel's (two chains on the 8-replica slice tables, merge, lane shift, row XOR);
// sums, header decode and verdict are rxv_kernel's, from the same window registers, with the
// geometry a loop invariant (fixed length). The frame's front lane stores the verdict.
// ---------------------------------------------------------------------------------------------
template <bool TRAILER>
__global__ __launch_bounds__(kDmaThreads, 1) void rxv_dma_kernel(RParams p) {
    using namespace fcs;
    constexpr int kWaves = kDmaThreads / 64;
    __shared__ __attribute__((aligned(16))) uint8_t lds[kDmaRing + kWaves * kDmaItemBytes];
    const int tid = threadIdx.x;
    if (TRAILER) {
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
    const uint32_t h = (uint32_t)(lane >> 3) & 3u, r4 = (uint32_t)(lane & 7) * 4u;
    const uint32_t B[4] = {r4 + 32u * (0u ^ h), r4 + 32u * (1u ^ h), r4 + 32u * (2u ^ h), r4 + 32u * (3u ^ h)};
    const uint32_t SEL[4] = {0x0C0C0400u + ((0u ^ h) << 8), 0x0C0C0400u + ((1u ^ h) << 8),
                             0x0C0C0400u + ((2u ^ h) << 8), 0x0C0C0400u + ((3u ^ h) << 8)};
    const uint32_t lanebase = kDmaHole + (uint32_t)(lane & 31) * 4u;

    // loop invariants: the window's place in the frame, leading bytes to mask, INV start
    const uint32_t ec = dma_end_off(c);
    const int rel = (int)p.flen - (int)ec - kChunkBytes;   // frame position of the window's first byte (>= -28)
    const int zc = (c == kGroup - 1) ? (int)(kDmaCover - p.flen) : (dma_short_lane(c) ? 4 : 0);
    const uint32_t x0 = (TRAILER && c == kGroup - 1)
                            ? lds_rd(lds, dma_hole(kDmaInvHole + (uint32_t)zc / 32u) + (uint32_t)(zc % 32) * 4u)
                            : 0u;

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
        // a frame past the batch's end (last item) works on the item's first frame: nothing outside the slot is read
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

        const Hdr H = decode<TRAILER>(fr, ch, c);
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
        uint32_t v = H.bits;
        if (TRAILER) {
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
            const uint32_t crc = row_xor(lane_shift_dma(lds, mv, lanebase));
            if (~crc != kResidue) v |= kFcsBad;
        }
        const uint32_t te = fold64(row_sum(fold64(tot))), ta = fold64(row_sum(fold64(tail)));
        const uint32_t hm = fold64(row_sum(H.sums & 0xffffu)), h0 = fold64(row_sum(H.sums >> 16));
        const bool oe = p.flen & 1u, om = fr.start & 1ull;
        const uint32_t tot_s = oe ? swap16(te) : te, tail_s = oe ? swap16(ta) : ta;
        const uint32_t hdr_s = om ? swap16(hm) : hm, head_s = om ? swap16(h0) : h0;
        if ((v & (kIpv4 | kIpBadHdr)) == kIpv4 && fold64(0xffffull + hdr_s) != 0xffffu) v |= kIpBadCsum;
        if (H.ps) {
            const uint64_t l4 = (uint64_t)H.ps + tot_s + (0xffffu - head_s) + (0xffffu - tail_s);
            if (fold64(l4) != 0xffffu) v |= kL4BadCsum;
        }
        const bool st = c == kGroup - 1 && f < p.n;
        if (st) p.verdict[f] = v;
        const uint64_t mb = __ballot(st && (v & p.bad_mask) != 0u);
        if (mb != 0 && lane == 0) *wave_bad<kDmaBad>(lds) += (uint64_t)__popcll(mb);
        it = nxt;
    }
    if (p.bad != nullptr && lane == 0) {
        const uint64_t b = *wave_bad<kDmaBad>(lds);
        if (b) atomicAdd(p.bad, (unsigned long long)b);
    }
}

// The one routing decision (launch_rxv launches what it returns; the engine leases a work counter
// exactly when it returns kDma).
Route route(bool var, const RParams &p, uint64_t dma_min) {
    if (!p.n) return Route::kNone;
    if (var || p.n <= dma_min) return Route::kGeneral;
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

hipError_t launch_rxv(bool var, bool trailer, const RParams &p, int cus, uint64_t dma_min, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    const Route rt = route(var, p, dma_min);
    if (rt == Route::kNone) return hipSuccess;
    g_last_route.store((int)rt, std::memory_order_relaxed);
    if (rt == Route::kDma) {
        if (!p.ctr) return hipErrorInvalidValue;
        const uint64_t items = (p.n + 3) / 4, wantd = (items + kDmaThreads / 64 - 1) / (kDmaThreads / 64);
        const int gd = (int)(wantd < (uint64_t)cus ? wantd : (uint64_t)cus);
        if (trailer) hipLaunchKernelGGL((rxv_dma_kernel<true>), dim3(gd), dim3(kDmaThreads), 0, st, p);
        else hipLaunchKernelGGL((rxv_dma_kernel<false>), dim3(gd), dim3(kDmaThreads), 0, st, p);
        return hipGetLastError();
    }
    const bool tiny = p.hi4 - p.lo4 < 2 * (uint64_t)kChunkBytes;
    // one workgroup per CU, persistent over the frames (a quarter-wave per frame)
    const uint64_t slots = kThreads / kGroup, want = (p.n + slots - 1) / slots;
    const int grid = (int)(want < (uint64_t)cus ? want : (uint64_t)cus);
#define RXV_GO(V, T, S) hipLaunchKernelGGL((rxv_kernel<V, T, S, kThreads>), dim3(grid), dim3(kThreads), 0, st, p)
    if (var) {
        if (trailer) { if (tiny) RXV_GO(true, true, true); else RXV_GO(true, true, false); }
        else { if (tiny) RXV_GO(true, false, true); else RXV_GO(true, false, false); }
    } else {
        if (trailer) { if (tiny) RXV_GO(false, true, true); else RXV_GO(false, true, false); }
        else { if (tiny) RXV_GO(false, false, true); else RXV_GO(false, false, false); }
    }
#undef RXV_GO
    return hipGetLastError();
}

}  // namespace rxv
