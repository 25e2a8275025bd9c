// dmx_kernel.hip — one-pass RX demultiplexing for gfx950: IPv4 datagrams in, per-socket queues of
// struct nstack_dgram records out, every payload byte read once and written once
// (include/nstack_dmx.h has the rules and the reference lines they restate).
//
// The build kernel. After the plan every datagram is independent: it writes one record at
// q + rec[k]. A QUARTER-WAVE takes a datagram; rows take runs of kRun consecutive datagrams from a
// zeroed device counter (row_work.hpp). The copy loop is rxr_kernel's, written again here (one shared
// loop changed the code of rxr_kernel's plain and summing builds and slowed them: DESIGN §3.19):
//   * The 24-byte header goes out as six aligned dword stores: the record start is a multiple of
//     align >= 8 behind a q aligned to it.
//   * The payload destination is rec + 24, so its phase on the 16-byte grid is 8 (0 or 8 at
//     align = 8). It is cut at that grid: the bytes in front and behind go out as byte stores (one
//     per lane), the 16-byte pieces between them as 16-byte stores, lane j piece j, j + 16, ... with
//     four pieces in flight. A piece's source is 16 bytes at any alignment: the four dwords from
//     floor4(source), a fifth where the source is not dword-aligned, joined by v_alignbyte. The
//     window of a piece stays inside the dword hull of the payload, which lies inside the datagram,
//     which was checked to lie inside `out`.
//   * The zero pad behind the payload: bytes up to the 8-byte grid, then one 8-byte store per lane
//     (the pad is shorter than align <= 128 = 16 lanes of 8 bytes; the record's end is 8-aligned).
//   No store touches a byte outside the record, every byte of it is stored once, and no dword is
//   read, modified and written back.
//
// The plan kernels follow below: table build, classify, the radix passes (histogram, scan, scatter),
// the scan of the record sizes in sorted order, and the per-socket search. No workgroup waits for
// another; data passes between the phases only across kernel boundaries; every probe loop is bounded
// by the table size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "dmx_launch.hpp"
#include "row_work.hpp"

namespace dmx {

using plan::block_scan_incl;
using row::gload;
using row::gstore;
using row::kFlight;
using row::kGroup;
using row::u32x4a4;
using row::kRun;

__device__ __forceinline__ uint64_t count_of(const DParams &p) {
    const uint64_t m = p.counts[0];
    return m < p.n ? m : p.n;
}

template <int NT>
__global__ __launch_bounds__(NT) void dmx_kernel(DParams p) {
    const int j = threadIdx.x & (kGroup - 1);
    const uint64_t m = count_of(p);
    // a row takes runs of datagrams from p.ctr
    row::for_each_item(p.ctr, p.n, [&](uint64_t k) {
        uint32_t fin = 0u;   // entries [m, n) are zero
        if (k < m) {
            const uint32_t st = p.pstat[k];
            fin = st;
            if (st & kQueued) {
                // whatever the plan arrays say, nothing outside the datagram inside `out` is read and
                // nothing outside the record's own range inside q is written
                const uint64_t at = p.doff[k], r = p.rec[k];
                const Cls c = classify(at, p.dlen[k], p.out_bytes, false, [&](uint64_t i) { return gload<uint8_t>(p.out + i); });
                const uint64_t size = rec_size(c.P, p.align);
                const bool ok = c.status == 0u && (r & (uint64_t)(p.align - 1u)) == 0ull && has_room(r, size, p.q_bytes);
                if (!ok) {
                    fin |= kNoRoom;
                } else {
                    fin |= kDelivered;
                    const uint64_t qa = p.q + r;
                    if (j < 6) {   // rule 6: struct nstack_dgram's 24 bytes
                        const uint32_t w = j == 0 ? c.src : j == 1 ? c.sport : j == 2 ? c.dst : j == 3 ? c.dport : j == 4 ? c.P : 0u;
                        gstore<uint32_t>(qa + 4u * (uint32_t)j, w);
                    }
                    const uint64_t s0 = p.out + at + c.pay, dA = qa + kRecHdr;
                    const uint32_t nb = c.P;
                    // ---- the bytes in front of the destination's first 16-byte line ----
                    uint32_t nh = (16u - ((uint32_t)dA & 15u)) & 15u;
                    nh = nh < nb ? nh : nb;
                    if ((uint32_t)j < nh) gstore<uint8_t>(dA + (uint32_t)j, gload<uint8_t>(s0 + (uint32_t)j));
                    // ---- whole 16-byte lines ----
                    const uint32_t nblk = (nb - nh) >> 4;
                    const uint64_t sb = s0 + nh, db = dA + nh;
                    const uint32_t rs = (uint32_t)sb & 3u;
                    for (uint32_t b0 = (uint32_t)j; b0 < nblk; b0 += kGroup * kFlight) {
                        u32x4a4 x[kFlight];
                        uint32_t x4[kFlight];
#pragma unroll
                        for (int f = 0; f < kFlight; f++) {
                            const uint32_t b = b0 + (uint32_t)(kGroup * f);
                            x[f] = u32x4a4{0u, 0u, 0u, 0u};
                            x4[f] = 0u;
                            if (b < nblk) {
                                const uint64_t a4 = (sb + 16ull * b) & ~3ull;
                                x[f] = gload<u32x4a4>(a4);
                                if (rs) x4[f] = gload<uint32_t>(a4 + 16);
                            }
                        }
#pragma unroll
                        for (int f = 0; f < kFlight; f++) {
                            const uint32_t b = b0 + (uint32_t)(kGroup * f);
                            if (b < nblk) {
                                u32x4a4 y;
                                y.x = __builtin_amdgcn_alignbyte(x[f].y, x[f].x, rs);
                                y.y = __builtin_amdgcn_alignbyte(x[f].z, x[f].y, rs);
                                y.z = __builtin_amdgcn_alignbyte(x[f].w, x[f].z, rs);
                                y.w = __builtin_amdgcn_alignbyte(x4[f], x[f].w, rs);
                                gstore<u32x4a4>(db + 16ull * b, y);
                            }
                        }
                    }
                    // ---- the bytes behind the last whole line ----
                    const uint32_t pt = nh + 16u * nblk + (uint32_t)j;
                    if (pt < nb) gstore<uint8_t>(dA + pt, gload<uint8_t>(s0 + pt));
                    // ---- the zero pad: [e0, rend), shorter than align; rend is a multiple of 8 ----
                    const uint64_t e0 = dA + nb, rend = qa + size;
                    const uint32_t zf = (8u - ((uint32_t)e0 & 7u)) & 7u;   // e0 <= rend, so e0 + zf <= rend
                    if ((uint32_t)j < zf) gstore<uint8_t>(e0 + (uint32_t)j, (uint8_t)0);
                    const uint64_t e8 = e0 + zf;
                    const uint32_t n8 = (uint32_t)((rend - e8) >> 3);      // at most 15
                    if ((uint32_t)j < n8) gstore<uint64_t>(e8 + 8u * (uint32_t)j, 0ull);
                }
            }
        }
        if (j == 0 && p.dstat != nullptr) p.dstat[k] = fin;
    });
}

// ---------------------------------------------------------------------------------------------
// The plan.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t hash_of(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
}

// 1. Every valid bind key claims or joins its entry; the lowest index stays (tidx starts at all ones).
// At most S <= tsize / 2 claims: the table cannot fill.
__global__ __launch_bounds__(kPlanThreads) void dmx_table_kernel(DParams p, Scratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.S) return;
    const unsigned long long key = p.bind[i];
    if (!key_valid(key)) return;   // matches nothing
    plan::probe(s.tsize, hash_of(key), [&](uint64_t h) {
        const unsigned long long old = atomicCAS(&s.tkey[h], 0ull, key);
        if (old != 0ull && old != key) return false;
        atomicMin(&s.tidx[h], (uint32_t)i);
        return true;
    });
}

// The lowest index of `key`, or kNone32. At most tsize probes; an empty entry ends every miss.
__device__ __forceinline__ uint32_t find(const Scratch &s, uint64_t key) {
    uint32_t idx = kNone32;
    plan::probe(s.tsize, hash_of(key), [&](uint64_t h) {
        const unsigned long long c = s.tkey[h];
        if (c == 0ull) return true;
        if (c != key) return false;
        idx = s.tidx[h];
        return true;
    });
    return idx;
}

// 2. Rules 1-6 for datagram k; the counters (integer adds commute: no order dependence).
__global__ __launch_bounds__(kPlanThreads) void dmx_classify_kernel(DParams p, Scratch s) {
    __shared__ unsigned int wg[3];
    if (threadIdx.x < 3) wg[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const uint64_t m = count_of(p);
    uint32_t st = 0u, sock = kNone32, size = 0u;
    if (k < m) {
        const bool badv = p.dverdict != nullptr && (p.dverdict[k] & (p.drop_mask | kDgNoRoom)) != 0u;
        const Cls c = classify(p.doff[k], p.dlen[k], p.out_bytes, badv, [&](uint64_t i) { return gload<uint8_t>(p.out + i); });
        st = c.status;
        if (!(st & (kDropped | kNoProto | kShort))) {   // rule 5
            sock = find(s, key_of(c.proto, c.dport, c.dst));
            if (sock == kNone32) st |= kNoSock;
        }
        if (st == 0u) {                                 // rule 6
            st = kQueued;
            size = (uint32_t)rec_size(c.P, p.align);
        }
    }
    if (k < p.n) {
        p.dstat[k] = st;
        p.dsock[k] = sock;
        p.rec[k] = kNone64;
        s.skey[k] = (st & kQueued) ? sock : kNone32;
        s.rsize[k] = size;
    }
    const uint64_t bq = __ballot((st & kQueued) != 0u), bn = __ballot((st & kNoSock) != 0u), bd = __ballot((st & kDropped) != 0u);
    if ((threadIdx.x & 63) == 0) {
        if (bq) atomicAdd(&wg[0], (unsigned int)__popcll(bq));
        if (bn) atomicAdd(&wg[1], (unsigned int)__popcll(bn));
        if (bd) atomicAdd(&wg[2], (unsigned int)__popcll(bd));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (wg[0]) atomicAdd((unsigned long long *)p.qcounts + 0, (unsigned long long)wg[0]);
        if (wg[1]) atomicAdd((unsigned long long *)p.qcounts + 2, (unsigned long long)wg[1]);
        if (wg[2]) atomicAdd((unsigned long long *)p.qcounts + 3, (unsigned long long)wg[2]);
    }
}

// 3a. The digit histogram of a tile: hist[digit * tiles + tile]. A key of kNone32 is no element.
__global__ __launch_bounds__(kPlanThreads) void dmx_hist_kernel(const uint32_t *keys, uint32_t shift, uint32_t *hist, uint64_t n,
                                                                uint64_t ntiles) {
    __shared__ unsigned int h[256];
    h[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
#pragma unroll
    for (int r = 0; r < (int)(kTile / kPlanThreads); r++) {
        const uint64_t i = base + (uint64_t)r * kPlanThreads + threadIdx.x;
        const uint32_t key = i < n ? keys[i] : kNone32;
        if (key != kNone32) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(uint64_t)threadIdx.x * ntiles + blockIdx.x] = h[threadIdx.x];
}

// 3b. One workgroup: the (digit, tile) counts become the counts in front, in the form of
// rxr_scan_totals_kernel. The sum is at most n < 2^30.
// A thread takes kScanPer consecutive entries a step, so that the workgroup-wide scan (sixteen
// barriers) is paid once per 4096 entries.
constexpr int kScanPer = 16;
__global__ __launch_bounds__(kPlanThreads) void dmx_scan_hist_kernel(uint32_t *hist, uint64_t entries) {
    __shared__ uint32_t sh[kPlanThreads];
    uint32_t base = 0u;
    for (uint64_t b0 = 0; b0 < entries; b0 += (uint64_t)kPlanThreads * kScanPer) {
        const uint64_t b = b0 + (uint64_t)threadIdx.x * kScanPer;
        uint32_t v[kScanPer], sum = 0u;
#pragma unroll
        for (int q = 0; q < kScanPer; q++) {
            v[q] = b + q < entries ? hist[b + q] : 0u;
            sum += v[q];
        }
        uint32_t tot;
        uint32_t at = base + block_scan_incl(sum, sh, tot) - sum;
#pragma unroll
        for (int q = 0; q < kScanPer; q++) {
            if (b + q < entries) hist[b + q] = at;
            at += v[q];
        }
        base += tot;
    }
}

// 3c. The scatter. An element's place is its (digit, tile) base plus its stable rank inside the tile:
// the elements of its digit in earlier rounds of the tile (run), in earlier waves of its round (cnt)
// and in lower lanes of its wave (eight ballots, one per digit bit). vals_in null: the element's own
// index.
__global__ __launch_bounds__(kPlanThreads) void dmx_scatter_kernel(const uint32_t *keys_in, const uint32_t *vals_in, uint32_t shift,
                                                                   const uint32_t *hist, uint32_t *keys_out, uint32_t *vals_out,
                                                                   uint64_t n, uint64_t ntiles) {
    constexpr int kWaves = kPlanThreads / 64;
    __shared__ uint32_t run[256];
    __shared__ uint32_t cnt[kWaves][256];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    run[t] = hist[(uint64_t)t * ntiles + blockIdx.x];
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    for (int r = 0; r < (int)(kTile / kPlanThreads); r++) {
#pragma unroll
        for (int q = 0; q < kWaves; q++) cnt[q][t] = 0u;
        __syncthreads();
        const uint64_t i = base + (uint64_t)r * kPlanThreads + t;
        const uint32_t key = i < n ? keys_in[i] : kNone32;
        const bool valid = key != kNone32;
        const uint32_t d = (key >> shift) & 255u;
        uint64_t same = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (d >> b) & 1u;
            const uint64_t bb = __ballot(valid && bit);
            same &= bit ? bb : ~bb;
        }
        const uint32_t lower = (uint32_t)__popcll(same & ((1ull << lane) - 1ull));
        if (valid && lower == 0u) cnt[w][d] = (uint32_t)__popcll(same);
        __syncthreads();
        if (valid) {
            uint32_t pos = run[d] + lower;
#pragma unroll
            for (int q = 0; q < kWaves; q++)
                if (q < w) pos += cnt[q][d];
            if (pos < n) {   // (always: the scan's total is at most n)
                keys_out[pos] = key;
                vals_out[pos] = vals_in != nullptr ? vals_in[i] : (uint32_t)i;
            }
        }
        __syncthreads();
        uint32_t add = 0u;
#pragma unroll
        for (int q = 0; q < kWaves; q++) add += cnt[q][t];
        run[t] += add;
    }
}

// 4a. The record size at a sorted position, and the block totals.
__device__ __forceinline__ uint64_t size_at(const Scratch &s, const uint32_t *keys, const uint32_t *idx, uint64_t pos, uint64_t n) {
    if (pos >= n || keys[pos] == kNone32) return 0ull;
    const uint32_t k = idx[pos];
    return k < n ? s.rsize[k] : 0ull;
}

__global__ __launch_bounds__(kPlanThreads) void dmx_size_totals_kernel(DParams p, Scratch s, const uint32_t *keys, const uint32_t *idx) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t pos = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    uint64_t tot;
    block_scan_incl(size_at(s, keys, idx, pos, p.n), sh, tot);
    if (threadIdx.x == 0) s.tot[blockIdx.x] = tot;
}

// 4b. One workgroup: the block totals become the sums of the blocks in front; sbase[S] and qcounts[1].
__global__ __launch_bounds__(kPlanThreads) void dmx_scan_totals_kernel(DParams p, Scratch s, uint64_t nb) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t base = plan::scan_totals(s.tot, nb, sh);
    if (threadIdx.x == 0) {
        p.sbase[p.S] = base;
        p.qcounts[1] = base;
    }
}

// 4c. rec: sockets are contiguous in sorted order, so the exclusive scan of the sizes is the offset.
__global__ __launch_bounds__(kPlanThreads) void dmx_place_kernel(DParams p, Scratch s, const uint32_t *keys, const uint32_t *idx) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t pos = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const uint64_t v = size_at(s, keys, idx, pos, p.n);
    const uint64_t at = s.tot[blockIdx.x] + plan::block_scan_excl(v, sh);
    if (pos < p.n && keys[pos] != kNone32 && idx[pos] < p.n) p.rec[idx[pos]] = at;
}

// The first sorted position whose key is >= s: at most 32 halvings of [0, n).
__device__ __forceinline__ uint64_t first_at_least(const uint32_t *keys, uint64_t n, uint32_t s) {
    uint64_t lo = 0, hi = n;
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < s) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// 5. sbase[s] and scnt[s], one socket per thread, behind the launch that stored rec.
__global__ __launch_bounds__(kPlanThreads) void dmx_sbase_kernel(DParams p, const uint32_t *keys, const uint32_t *idx) {
    const uint64_t sck = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (sck >= p.S) return;
    const uint64_t lo = first_at_least(keys, p.n, (uint32_t)sck), hi = first_at_least(keys, p.n, (uint32_t)sck + 1u);
    p.scnt[sck] = (uint32_t)(hi - lo);
    const bool some = lo < p.n && keys[lo] != kNone32 && idx[lo] < p.n;
    p.sbase[sck] = some ? p.rec[idx[lo]] : p.qcounts[1];
}

namespace {
std::atomic<int> g_last_route{(int)Route::kNone};
}
Route last_launch() { return (Route)g_last_route.load(std::memory_order_relaxed); }

hipError_t launch_build(const DParams &p, int cus, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (!p.n) return hipSuccess;
    if (!p.ctr) return hipErrorInvalidValue;
    // four workgroups per CU at the most, persistent over the datagrams
    const uint64_t rows = kThreads / kGroup, want = (p.n + rows * kRun - 1) / (rows * kRun);
    const uint64_t most = (uint64_t)cus * 4;
    const int grid = (int)(want < most ? want : most);
    g_last_route.store((int)Route::kDemux, std::memory_order_relaxed);
    hipLaunchKernelGGL((dmx_kernel<kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_plan(const DParams &p, const Scratch &s, hipStream_t st) {
    (void)hipGetLastError();
    if (!p.n) return hipSuccess;
    const uint64_t nb = plan_blocks(p.n), nt = tiles(p.n);
    if (nb > 0x7fffffffull || p.n >= kMaxDgs) return hipErrorInvalidValue;
    const dim3 t(kPlanThreads), g((unsigned)nb), gt((unsigned)nt);
    if (p.S) PLAN_LAUNCH(dmx_table_kernel, dim3((unsigned)plan_blocks(p.S)), t, 0, st, p, s);
    PLAN_LAUNCH(dmx_classify_kernel, g, t, 0, st, p, s);
    PLAN_LAUNCH(dmx_hist_kernel, gt, t, 0, st, s.skey, 0u, s.hist, p.n, nt);
    PLAN_LAUNCH(dmx_scan_hist_kernel, dim3(1), t, 0, st, s.hist, nt * 256);
    PLAN_LAUNCH(dmx_scatter_kernel, gt, t, 0, st, s.skey, (const uint32_t *)nullptr, 0u, s.hist, s.key1, s.idx1, p.n, nt);
    const uint32_t *keys = s.key1, *idx = s.idx1;
    if (p.S > 256u) {
        PLAN_LAUNCH(dmx_hist_kernel, gt, t, 0, st, s.key1, 8u, s.hist, p.n, nt);
        PLAN_LAUNCH(dmx_scan_hist_kernel, dim3(1), t, 0, st, s.hist, nt * 256);
        PLAN_LAUNCH(dmx_scatter_kernel, gt, t, 0, st, s.key1, s.idx1, 8u, s.hist, s.key2, s.idx2, p.n, nt);
        keys = s.key2;
        idx = s.idx2;
    }
    PLAN_LAUNCH(dmx_size_totals_kernel, g, t, 0, st, p, s, keys, idx);
    PLAN_LAUNCH(dmx_scan_totals_kernel, dim3(1), t, 0, st, p, s, nb);
    PLAN_LAUNCH(dmx_place_kernel, g, t, 0, st, p, s, keys, idx);
    if (p.S) PLAN_LAUNCH(dmx_sbase_kernel, dim3((unsigned)plan_blocks(p.S)), t, 0, st, p, keys, idx);
    return hipSuccess;
}

}  // namespace dmx
