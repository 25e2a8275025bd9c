// gro_kernel.hip — the plan of one-pass RX coalescing for gfx950 (include/nstack_gro.h has the
// rules): which in-order TCP segments of a batch leave as one large datagram.
//
// The launches sit between those of the reassembly plan (rxr_kernel.hip), whose classify, insert and
// link run first and whose scan, place and finish run behind its decide launch:
//   classify  rule 2 on every RXR_WHOLE frame: GRO_CAND and the segment record;
//   insert    every candidate claims or joins the entry of its (flow, seq) and the entry of its
//             group (flow, seq >> 15); the group's accumulator lives on the frame that claimed the
//             latter and takes the lowest seq and the member count;
//   link      every candidate looks its successor up (the member whose seq is its end, in the same
//             window) and adds itself up: rules 3a, 3b, 3c and the FIN / PSH half of 3e;
//   first     the minimum has settled across the kernel boundary: every candidate looks up
//             (flow, lowest seq), the first member, and compares its headers with it: rule 3d and
//             the CWR half of 3e;
//   [rxr decide<GRO>, scan, place, finish]
//   finish    every member of a coalescible group takes its bits, and the members behind the first
//             their place behind the first's.
// One frame per thread; no workgroup waits for another; data passes between the phases only across
// kernel boundaries; every probe loop is bounded by the table size, and neither table can fill (at
// most n claims in at least 2 n entries each).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcs_crc.hpp"
#include "gro_launch.hpp"

namespace gro {

using fcs::gload;
using rxr::Entry;
using rxr::kNone32;
using plan::kPlanThreads;
using rxr::RParams;
using rxr::Scratch;

__device__ __forceinline__ bool same_flow(const GRec &a, const GRec &b) {
    return a.src == b.src && a.dst == b.dst && a.ports == b.ports;
}

// The entry of (me's flow, seq) in the seq table, or tsize when there is none. At most tsize probes;
// the table holds at most n <= tsize / 2 claims, so an empty entry ends every miss.
__device__ __forceinline__ uint64_t find_seq(const GScratch &g, const GRec &me, uint32_t seq) {
    uint64_t at = g.tsize;
    plan::probe(g.tsize, plan::mix4(me.src, me.dst, me.ports, seq), [&](uint64_t h) {
        const uint32_t c = g.tabs[h].claim;
        if (c == 0u) return true;
        const GRec o = g.rec[c - 1u];
        if (!(same_flow(o, me) && o.seq == seq)) return false;
        at = h;
        return true;
    });
    return at;
}

__device__ __forceinline__ uint32_t hlen_of(uint32_t w4) { return ((w4 >> 20) & 0x0fu) * 4u; }
__device__ __forceinline__ uint32_t thl_of(uint32_t w4) { return ((w4 >> 16) & 0x0fu) * 4u; }

// 1. Rule 2 and the segment record. A whole frame lies inside the arena (rxr classify), and
// candidate() asks only for bytes of its TCP header once that is known to lie inside the datagram.
__global__ __launch_bounds__(kPlanThreads) void gro_classify_kernel(RParams p, Scratch s, GScratch g) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t st = p.fstat[i];
    if (!(st & rxr::kWhole)) return;
    const rxr::Rec rc = s.rec[i];
    const uint32_t hlen = ((rc.w2 >> 25) & 0x0fu) * 4u, I = rc.w3 >> 16, proto = (rc.w2 >> 16) & 0xffu;
    const uint64_t ip = p.base + p.off[i] + 14u;
    Seg sg{0u, 0u, 0u, 0u, 0u};
    if (!candidate(proto, hlen, I, [&](uint32_t q) { return (uint32_t)gload<uint8_t>(ip + q); }, sg)) return;
    p.fstat[i] = st | kCand;
    GRec r;
    r.src = rc.src;
    r.dst = rc.dst;
    r.ports = sg.ports;
    r.seq = sg.seq;
    r.w4 = sg.P | ((sg.thl >> 2) << 16) | ((hlen >> 2) << 20) | (sg.tflags << 24);
    r.group = kNone32;
    r.first = kNone32;
    r.pad = 0u;
    g.rec[i] = r;
}

// 2. Every candidate claims or joins the entries of its (flow, seq) and of its group.
__global__ __launch_bounds__(kPlanThreads) void gro_insert_kernel(RParams p, GScratch g) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n || !(p.fstat[i] & kCand)) return;
    const GRec me = g.rec[i];
    plan::probe(g.tsize, plan::mix4(me.src, me.dst, me.ports, me.seq), [&](uint64_t h) {
        const uint32_t old = atomicCAS(&g.tabs[h].claim, 0u, (uint32_t)i + 1u);
        if (old != 0u) {
            const GRec o = g.rec[old - 1u];
            if (!(same_flow(o, me) && o.seq == me.seq)) return false;
        }
        atomicAdd(&g.tabs[h].count, 1u);
        return true;
    });
    const uint32_t win = me.seq >> kWinShift;
    plan::probe(g.tsize, plan::mix4(me.src, me.dst, me.ports, win ^ 0xA5A50000u), [&](uint64_t h) {
        const uint32_t old = atomicCAS(&g.tabg[h].claim, 0u, (uint32_t)i + 1u);
        uint32_t c = (uint32_t)i;
        if (old != 0u) {
            const GRec o = g.rec[old - 1u];
            if (!(same_flow(o, me) && (o.seq >> kWinShift) == win)) return false;
            c = old - 1u;
        }
        g.rec[i].group = c;   // no other thread reads or writes this word in this launch
        atomicMax(&g.acc[c].invmin, kWin - (me.seq & (kWin - 1u)));
        atomicAdd(&g.acc[c].members, 1u);
        return true;
    });
}

// 3. Every candidate finds its successor and adds itself up on the group's accumulator.
__global__ __launch_bounds__(kPlanThreads) void gro_link_kernel(RParams p, GScratch g) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n || !(p.fstat[i] & kCand)) return;
    const GRec me = g.rec[i];
    if (me.group >= p.n) return;
    GAcc *a = g.acc + me.group;
    const uint32_t P = me.w4 & 0xffffu, tf = me.w4 >> 24, end = me.seq + P;   // mod 2^32
    const uint64_t own = find_seq(g, me, me.seq);
    bool fault = own == g.tsize || g.tabs[own].count != 1u;                     // 3a: two members with the same seq
    // 3b: a successor is a member of this group: its seq lies in the same window
    const bool succ = (end >> kWinShift) == (me.seq >> kWinShift) && find_seq(g, me, end) != g.tsize;
    if (succ) {
        fault = fault || (tf & (kTcpFin | kTcpPsh));                            // 3e: FIN or PSH in front of the last
    } else {
        atomicAdd(&a->lasts, 1u);
        atomicMax(&a->maxend, (me.seq & (kWin - 1u)) + P);
        atomicOr(&a->lastflags, tf & (kTcpFin | kTcpPsh));
    }
    atomicAdd(&a->sumP, (unsigned long long)P);
    if (fault) atomicOr(&a->fault, 1u);
}

// 4. Every candidate of a group of two or more finds the first member and compares itself with it.
__global__ __launch_bounds__(kPlanThreads) void gro_first_kernel(RParams p, GScratch g) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n || !(p.fstat[i] & kCand)) return;
    const GRec me = g.rec[i];
    if (me.group >= p.n) return;
    GAcc *a = g.acc + me.group;
    if (a->members < 2u) return;
    const uint32_t fseq = (me.seq & ~(kWin - 1u)) | (kWin - a->invmin);
    const uint64_t e = find_seq(g, me, fseq);
    if (e == g.tsize) return;   // (the lowest seq is a member's: cannot happen)
    const uint32_t f = g.tabs[e].claim - 1u;
    g.rec[i].first = f;         // no other thread reads or writes this word in this launch
    if (f == (uint32_t)i) return;
    const GRec fr = g.rec[f];
    bool fault = ((me.w4 ^ fr.w4) & 0x00ff0000u) != 0u || ((me.w4 >> 24) & kTcpCwr);   // 3d: hlen, thl; 3e: CWR
    if (!fault) {
        const uint64_t ia = p.base + p.off[f] + 14u, ib = p.base + p.off[i] + 14u;
        fault = !compatible([&](uint32_t q) { return (uint32_t)gload<uint8_t>(ia + q); },
                            [&](uint32_t q) { return (uint32_t)gload<uint8_t>(ib + q); }, hlen_of(fr.w4), thl_of(fr.w4));
    }
    if (fault) atomicOr(&a->fault, 1u);
}

// 6. Finish (rule 4 and 5): the members of a coalescible group take their bits; the first was placed
// by the place launch, the others go behind it. Only members behind the first are written here, and
// only firsts are read.
__global__ __launch_bounds__(kPlanThreads) void gro_finish_kernel(RParams p, GScratch g) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n) return;
    const uint32_t st = p.fstat[i];
    if (!(st & kCand)) return;
    const GRec me = g.rec[i];
    if (me.group >= p.n) return;
    const GAcc a = g.acc[me.group];
    if (!coalescible(a) || me.first >= p.n) return;
    if (me.first == (uint32_t)i) {
        p.fstat[i] = st | kMerged | rxr::kHead | last_bits(a.lastflags);
        return;
    }
    const GRec fr = g.rec[me.first];
    p.fstat[i] = st | kMerged;
    p.dgi[i] = p.dgi[me.first];
    p.dst[i] = p.dst[me.first] + hlen_of(fr.w4) + thl_of(fr.w4) + (me.seq - fr.seq);
}

hipError_t launch_plan(const RParams &p, const Scratch &s, const GScratch &g, hipStream_t st) {
    (void)hipGetLastError();
    if (!p.n) return hipSuccess;
    const uint64_t nb = plan::plan_blocks(p.n);
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 grid((unsigned)nb), t(kPlanThreads);
    hipError_t e;
    if ((e = rxr::launch_plan_front(p, s, st)) != hipSuccess) return e;
    PLAN_LAUNCH(gro_classify_kernel, grid, t, 0, st, p, s, g);
    PLAN_LAUNCH(gro_insert_kernel, grid, t, 0, st, p, g);
    PLAN_LAUNCH(gro_link_kernel, grid, t, 0, st, p, g);
    PLAN_LAUNCH(gro_first_kernel, grid, t, 0, st, p, g);
    if ((e = rxr::launch_plan_decide(p, s, &g, st)) != hipSuccess) return e;
    if ((e = rxr::launch_plan_back(p, s, st)) != hipSuccess) return e;
    PLAN_LAUNCH(gro_finish_kernel, grid, t, 0, st, p, g);
    return hipSuccess;
}

}  // namespace gro
