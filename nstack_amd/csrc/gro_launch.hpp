// gro_launch.hpp — host-side launchers of the plan of one-pass RX coalescing (gro_kernel.hip) and
// the scratch its launches share with the decide launch of rxr_kernel.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gro_plan.hpp"
#include "rxr_launch.hpp"

namespace gro {

// The plan's scratch on top of rxr::Scratch (device memory that lives on the stream between the launches).
struct GRec {   // the segment record of a candidate, written by the classify launch
    uint32_t src, dst, ports, seq;
    uint32_t w4;      // P | (thl / 4) << 16 | (hlen / 4) << 20 | TCP flags << 24
    uint32_t group;   // the frame that claimed (flow, seq >> 15): its GAcc is the group's (insert launch)
    uint32_t first;   // the group's first member, or kNone32 (first launch)
    uint32_t pad;
};
struct GAcc {   // what a group's members add up on the record of the frame that claimed (flow, window)
    unsigned long long sumP;
    uint32_t invmin;      // 0x8000 - the lowest seq & 0x7fff (a maximum, so that zero is "none yet")
    uint32_t maxend;      // the highest (seq & 0x7fff) + P among the members without a successor
    uint32_t lasts;       // members without a successor in the group
    uint32_t fault;       // rules 3a, 3d, 3e
    uint32_t members;
    uint32_t lastflags;   // FIN | PSH of the members without a successor
};
struct GScratch {
    GRec *rec;
    GAcc *acc;
    rxr::Entry *tabs;   // keyed by (flow, seq), with the arrival count
    rxr::Entry *tabg;   // keyed by (flow, seq >> 15)
    uint64_t tsize;     // of either table: a power of two, >= 2 n
};

// Rule 3 from a group's accumulator, once the insert, link and first launches have run.
RXR_HD bool coalescible(const GAcc &a) {
    return a.members >= 2u && a.fault == 0u && a.lasts == 1u &&
           a.sumP == (unsigned long long)(a.maxend - (kWin - a.invmin));
}

// Bytes of scratch behind rxr::scratch_bytes(n), its carving (16-byte aligned parts), and the part
// the plan wants zeroed before its first launch: acc and both tables (adjacent, in front).
inline uint64_t scratch_bytes(uint64_t n) { return n * (sizeof(GAcc) + sizeof(GRec)) + 2 * plan::table_size(n) * sizeof(rxr::Entry); }
inline uint64_t zeroed_bytes(uint64_t n) { return n * sizeof(GAcc) + 2 * plan::table_size(n) * sizeof(rxr::Entry); }
inline GScratch carve(void *mem, uint64_t n) {
    GScratch g;
    uint8_t *p = static_cast<uint8_t *>(mem);
    g.acc = reinterpret_cast<GAcc *>(p);
    p += n * sizeof(GAcc);
    g.tsize = plan::table_size(n);
    g.tabs = reinterpret_cast<rxr::Entry *>(p);
    p += g.tsize * sizeof(rxr::Entry);
    g.tabg = reinterpret_cast<rxr::Entry *>(p);
    p += g.tsize * sizeof(rxr::Entry);
    g.rec = reinterpret_cast<GRec *>(p);
    return g;
}

// The plan of p.n frames: the launches of include/nstack_gro.h on `st`. s and g are carved scratch
// whose zeroed parts have been zeroed on the stream.
hipError_t launch_plan(const rxr::RParams &p, const rxr::Scratch &s, const GScratch &g, hipStream_t st);

}  // namespace gro

namespace rxr {
// The pieces of launch_plan (rxr_kernel.hip), for gro::launch_plan: classify, insert, link; the
// decide launch (g: null for the plain plan); the scan of the totals, place, finish.
hipError_t launch_plan_front(const RParams &p, const Scratch &s, hipStream_t st);
hipError_t launch_plan_decide(const RParams &p, const Scratch &s, const gro::GScratch *g, hipStream_t st);
hipError_t launch_plan_back(const RParams &p, const Scratch &s, hipStream_t st);
}  // namespace rxr
