// mux_kernel.hip — one-pass TX multiplexing for gfx950: per-socket send queues of struct nstack_dgram
// records in, finished IPv4 datagrams out, every payload byte read once and written once
// (include/nstack_mux.h has the rules and the reference lines they restate).
//
// The build kernel. After the plan every record is independent: it writes one datagram at
// dgram + off[k]. A QUARTER-WAVE takes a record; rows take runs of kRun consecutive records from a
// zeroed device counter (row_work.hpp).
//   * The row loads the plan words, the record's header and the 40-byte image (lanes 0..9, one dword
//     each) and re-checks rule 8: whatever the plan arrays say, nothing outside the record inside q
//     is read and nothing outside [off, off + len) inside dgram is written.
//   * The hl header bytes (28 or 40) go out as aligned dword stores, lane j dword j: the datagram
//     start is a multiple of align >= 4 behind a dgram aligned to it.
//   * The payload source is rec + 24, phase 8 on the 16-byte grid of a q aligned to 16; the
//     destination is off + hl, any multiple of 4. copy16.hpp cuts it at the destination's grid.
//   No store touches a byte outside the datagram, every byte of it is stored once, the pad up to
//   align is not touched, and no dword is read, modified and written back.
//
// The plan kernels follow below: neighbour table, classify, block totals, their scan, place, tnext.
// No workgroup waits for another; data passes between the phases only across kernel boundaries;
// every probe loop is bounded by the table size.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "copy16.hpp"
#include "mux_launch.hpp"
#include "row_work.hpp"

namespace mux {

using plan::block_scan_incl;
using row::gload;
using row::gstore;
using row::kGroup;
using row::kRun;

template <int NT>
__global__ __launch_bounds__(NT) void mux_kernel(MParams p) {
    const int j = threadIdx.x & (kGroup - 1);
    // a row takes runs of records from p.ctr
    row::for_each_item(p.ctr, p.n, [&](uint64_t k) {
        const uint32_t st = p.pstat[k];
        uint32_t fin = st;
        if (st & kPlanned) {
            const uint64_t r = p.rec[k], at = p.off[k];
            const uint32_t len = p.len[k];
            const uint32_t *img = p.himg + k * kImgWords;
            const uint32_t w2 = img[2];
            const Rec c = read_rec(r, p.q_bytes, [&](uint64_t i) { return gload<uint32_t>(p.q + i); });
            if (!build_ok(c, at, len, w2, p.align, p.dgram_bytes)) {
                fin |= kNoRoom;
            } else {
                fin |= kBuilt;
                const uint32_t hl = hl_of(image_proto(w2));
                const uint64_t da = p.dgram + at;
                if ((uint32_t)j < hl / 4u) gstore<uint32_t>(da + 4u * (uint32_t)j, img[j]);   // rules 5, 7: the finished headers
                copy16::row_copy(p.q + r + kRecHdr, da + hl, (uint32_t)c.P, j);
            }
        }
        if (j == 0 && p.mstat != nullptr) p.mstat[k] = fin;
    });
}

// ---------------------------------------------------------------------------------------------
// The plan.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long nkey_of(uint32_t addr) { return (1ull << 32) | addr; }   // never 0: 0 is "empty"
__device__ __forceinline__ uint64_t hash_of(uint32_t addr) { return plan::mix4(addr, 0u, 0u, 0u); }

// 1. Every valid neighbour claims or joins its entry; the lowest index stays (tidx starts at all
// ones). At most N <= tsize / 2 claims: the table cannot fill.
__global__ __launch_bounds__(kPlanThreads) void mux_neigh_kernel(MParams p, Scratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.N) return;
    if (!p.nb[i].valid) return;   // matches nothing
    const unsigned long long key = nkey_of(p.nb[i].addr);
    plan::probe(s.tsize, hash_of(p.nb[i].addr), [&](uint64_t h) {
        const unsigned long long old = atomicCAS(&s.tkey[h], 0ull, key);
        if (old != 0ull && old != key) return false;
        atomicMin(&s.tidx[h], (uint32_t)i);
        return true;
    });
}

// The lowest valid index of `addr`, or kNone32. At most tsize probes; an empty entry ends every miss.
__device__ __forceinline__ uint32_t find_neigh(const Scratch &s, uint32_t addr) {
    uint32_t idx = kNone32;
    const unsigned long long key = nkey_of(addr);
    plan::probe(s.tsize, hash_of(addr), [&](uint64_t h) {
        const unsigned long long c = s.tkey[h];
        if (c == 0ull) return true;
        if (c != key) return false;
        idx = s.tidx[h];
        return true;
    });
    return idx;
}

// The socket whose range [sfirst[s], sfirst[s + 1]) holds k, or kNone32: at most 32 halvings of
// [0, S]; the range is checked, so an sfirst that is not monotone still gives a function of the inputs.
__device__ __forceinline__ uint32_t socket_of(const uint64_t *sfirst, uint32_t S, uint64_t k) {
    uint64_t lo = 0, hi = (uint64_t)S + 1;   // the first index whose sfirst lies behind k
    for (int it = 0; it < 32 && lo < hi; it++) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sfirst[mid] <= k) lo = mid + 1;
        else hi = mid;
    }
    if (lo < 1 || lo > S) return kNone32;
    const uint64_t s = lo - 1;
    return sfirst[s] <= k && k < sfirst[s + 1] ? (uint32_t)s : kNone32;
}

// 2. Rules 1-4 for record k; the counters (integer adds commute: no order dependence).
__global__ __launch_bounds__(kPlanThreads) void mux_classify_kernel(MParams p, Scratch s) {
    __shared__ uint32_t rnet[kMaxRoutes], rmask[kMaxRoutes];
    __shared__ unsigned int wg[3];
    static_assert(kMaxRoutes <= (uint32_t)kPlanThreads, "one route per thread stages the table");
    if (threadIdx.x < p.R) {
        rnet[threadIdx.x] = p.rt[threadIdx.x].network;
        rmask[threadIdx.x] = p.rt[threadIdx.x].netmask;
    }
    if (threadIdx.x < 3) wg[threadIdx.x] = 0u;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    uint32_t st = 0u, sock = kNone32, ri = kNone32, ni = kNone32, pad = 0u, tp = 0u;
    if (k < p.n) {
        st = kBadRec;
        sock = socket_of(p.sfirst, p.S, k);
        if (sock != kNone32) {
            const uint64_t key = p.bind[sock];
            const uint32_t proto = key_proto(key);
            const Rec c = read_rec(p.rec[k], p.q_bytes, [&](uint64_t i) { return gload<uint32_t>(p.q + i); });
            st = key_valid(key) ? c.status : kBadRec;
            if (!st) {                                       // rule 2
                if (!size_ok(proto, c.P)) st |= kBadSize;
                if (proto == 6u && p.tcb == nullptr) st |= kNoTcb;
            }
            if (!st) {                                       // rule 3
                ri = route_find(p.R, c.dst, [&](uint32_t i) { return rnet[i]; }, [&](uint32_t i) { return rmask[i]; });
                if (ri == kNone32) st = kNoRoute;
            }
            if (!st) {                                       // rule 4
                ni = find_neigh(s, c.dst);
                if (ni >= p.N) {
                    ni = kNone32;
                    st = kNoNeigh;
                }
            }
            if (!st) {                                       // rule 5
                st = kPlanned;
                pad = (uint32_t)padded(hl_of(proto) + (uint32_t)c.P, p.align);
                tp = proto == 6u ? (uint32_t)c.P : 0u;
            }
        }
        p.mstat[k] = st;
        s.sock[k] = sock;
        s.rti[k] = ri;
        s.nbi[k] = ni;
        s.pbytes[k] = pad;
        s.ptcp[k] = tp;
    }
    const uint64_t bp = __ballot((st & kPlanned) != 0u), br = __ballot((st & kNoRoute) != 0u), bn = __ballot((st & kNoNeigh) != 0u);
    if ((threadIdx.x & 63) == 0) {
        if (bp) atomicAdd(&wg[0], (unsigned int)__popcll(bp));
        if (br) atomicAdd(&wg[1], (unsigned int)__popcll(br));
        if (bn) atomicAdd(&wg[2], (unsigned int)__popcll(bn));
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (wg[0]) atomicAdd((unsigned long long *)p.counts + 0, (unsigned long long)wg[0]);
        if (wg[1]) atomicAdd((unsigned long long *)p.counts + 2, (unsigned long long)wg[1]);
        if (wg[2]) atomicAdd((unsigned long long *)p.counts + 3, (unsigned long long)wg[2]);
    }
}

// 3. The block totals of the three sums; each element keeps the sum of those in front of it inside
// its block (a block's padded sizes sum to less than 2^25).
__global__ __launch_bounds__(kPlanThreads) void mux_totals_kernel(MParams p, Scratch s) {
    __shared__ uint32_t sh[kPlanThreads];
    const uint64_t k = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const bool in = k < p.n;
    const uint32_t vb = in ? s.pbytes[k] : 0u, vt = in ? s.ptcp[k] : 0u, vr = in && (p.mstat[k] & kPlanned) ? 1u : 0u;
    uint32_t tb, tt, tr;
    const uint32_t ib = block_scan_incl(vb, sh, tb), it = block_scan_incl(vt, sh, tt), ir = block_scan_incl(vr, sh, tr);
    if (in) {
        s.pbytes[k] = ib - vb;
        s.ptcp[k] = it - vt;
        s.prank[k] = ir - vr;
    }
    if (threadIdx.x == 0) {
        s.totb[blockIdx.x] = tb;
        s.tott[blockIdx.x] = tt;
        s.totr[blockIdx.x] = tr;
    }
}

// 4. One workgroup: the block totals become the sums of the blocks in front; entry nb gets the sum of
// all, and counts[1] the bytes.
__global__ __launch_bounds__(kPlanThreads) void mux_scan_totals_kernel(MParams p, Scratch s, uint64_t nb) {
    __shared__ uint64_t sh64[kPlanThreads];
    __shared__ uint32_t sh32[kPlanThreads];
    const uint64_t bytes = plan::scan_totals(s.totb, nb, sh64);
    const uint32_t tcp = plan::scan_totals(s.tott, nb, sh32);
    const uint32_t rank = plan::scan_totals(s.totr, nb, sh32);
    if (threadIdx.x == 0) {
        s.totb[nb] = bytes;
        s.tott[nb] = tcp;
        s.totr[nb] = rank;
        p.counts[1] = bytes;
    }
}

// The TCP payload bytes of the planned records in front of position pos <= n.
__device__ __forceinline__ uint32_t tcp_before(const Scratch &s, uint64_t pos, uint64_t n) {
    return pos >= n ? s.tott[(n + kPlanThreads - 1) / kPlanThreads] : s.tott[pos / kPlanThreads] + s.ptcp[pos];
}

// 5. off, len, l2 and the header image of record k.
__global__ __launch_bounds__(kPlanThreads) void mux_place_kernel(MParams p, Scratch s) {
    const uint64_t k = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (k >= p.n) return;
    const uint32_t st = p.mstat[k];
    const uint64_t blk = k / kPlanThreads;
    p.off[k] = s.totb[blk] + s.pbytes[k];
    uint32_t w[kImgWords] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    uint32_t len = 0u;
    const uint32_t sock = s.sock[k], ri = s.rti[k], ni = s.nbi[k];
    const bool planned = (st & kPlanned) && sock < p.S && ri < p.R && ni < p.N;   // (always, for a planned record)
    uint8_t *l2 = reinterpret_cast<uint8_t *>(p.l2 + k);   // 12 bytes at any alignment
    if (planned) {
        const uint64_t r = p.q + p.rec[k], key = p.bind[sock];
        const uint32_t proto = key_proto(key), P = gload<uint32_t>(r + 16);
        Hdr h{proto, P, (p.id0 + s.totr[blk] + s.prank[k]) & 0xffffu, p.rt[ri].iface, gload<uint32_t>(r + 8), key_port(key),
              gload<uint32_t>(r + 12), 0u, 0u, 0u, 0u};
        if (proto == 6u && p.tcb != nullptr) {
            const mux_tcb t = p.tcb[sock];
            h.seq = t.seq + (tcp_before(s, k, p.n) - tcp_before(s, p.sfirst[sock], p.n));
            h.ack = t.ack;
            h.flags = t.flags;
            h.win = t.win;
        }
        make_image(h, w);
        len = hl_of(proto) + P;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            l2[i] = p.nb[ni].mac[i];
            l2[6 + i] = p.rt[ri].mac[i];
        }
    } else {
#pragma unroll
        for (int i = 0; i < 12; i++) l2[i] = 0;
    }
    p.len[k] = len;
#pragma unroll
    for (uint32_t i = 0; i < kImgWords; i++) p.himg[k * kImgWords + i] = w[i];
}

// 6. tnext[s], one socket per thread. n = 0: no record, and no scratch is read.
__global__ __launch_bounds__(kPlanThreads) void mux_tnext_kernel(MParams p, Scratch s) {
    const uint64_t sck = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (sck >= p.S) return;
    const uint64_t key = p.bind[sck];
    uint32_t v = 0u;
    if (key_valid(key) && key_proto(key) == 6u && p.tcb != nullptr) {
        v = p.tcb[sck].seq;
        if (p.n) {
            uint64_t a = p.sfirst[sck], b = p.sfirst[sck + 1];
            a = a < p.n ? a : p.n;
            b = b < p.n ? b : p.n;
            b = b < a ? a : b;
            v += tcp_before(s, b, p.n) - tcp_before(s, a, p.n);
        }
    }
    p.tnext[sck] = v;
}

namespace {
std::atomic<int> g_last_route{(int)Route::kNone};
}
Route last_launch() { return (Route)g_last_route.load(std::memory_order_relaxed); }

hipError_t launch_build(const MParams &p, int cus, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (!p.n) return hipSuccess;
    if (!p.ctr) return hipErrorInvalidValue;
    // four workgroups per CU at the most, persistent over the records
    const uint64_t rows = kThreads / kGroup, want = (p.n + rows * kRun - 1) / (rows * kRun);
    const uint64_t most = (uint64_t)cus * 4;
    const int grid = (int)(want < most ? want : most);
    g_last_route.store((int)Route::kMux, std::memory_order_relaxed);
    hipLaunchKernelGGL((mux_kernel<kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_plan(const MParams &p, const Scratch &s, hipStream_t st) {
    (void)hipGetLastError();
    const dim3 t(kPlanThreads);
    if (p.n) {
        const uint64_t nb = plan_blocks(p.n);
        if (nb > 0x7fffffffull || p.n >= kMaxRecs) return hipErrorInvalidValue;
        const dim3 g((unsigned)nb);
        if (p.N) PLAN_LAUNCH(mux_neigh_kernel, dim3((unsigned)plan_blocks(p.N)), t, 0, st, p, s);
        PLAN_LAUNCH(mux_classify_kernel, g, t, 0, st, p, s);
        PLAN_LAUNCH(mux_totals_kernel, g, t, 0, st, p, s);
        PLAN_LAUNCH(mux_scan_totals_kernel, dim3(1), t, 0, st, p, s, nb);
        PLAN_LAUNCH(mux_place_kernel, g, t, 0, st, p, s);
    }
    if (p.S && p.tnext) PLAN_LAUNCH(mux_tnext_kernel, dim3((unsigned)plan_blocks(p.S)), t, 0, st, p, s);
    return hipSuccess;
}

}  // namespace mux
