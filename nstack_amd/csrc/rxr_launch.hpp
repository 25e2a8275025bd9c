// rxr_launch.hpp — host-side launchers of one-pass RX reassembly (rxr_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_prims.hpp"
#include "rxr_plan.hpp"

namespace rxr {

// What the kernels read: frame i = [base + off[i], + len[i]); [lo4, hi4) is the readable range of
// the frame arena, dword-rounded.
struct RParams {
    uint64_t base, arena_bytes;
    uint64_t lo4, hi4;
    const uint64_t *off;
    const uint32_t *len;
    uint64_t n;
    uint32_t flags, align;
    // the plan
    const uint32_t *verdict;   // may be null
    uint32_t drop_mask;
    uint32_t *fstat;           // plan: out. build: the final word, may be null
    uint64_t *dst;
    uint32_t *dgi;
    uint64_t *doff;
    uint32_t *dlen;
    uint32_t *dlead;           // may be null
    uint64_t *counts;          // may be null
    // the build
    const uint32_t *pstat;
    uint64_t out, out_bytes;
    unsigned long long *ctr;   // zeroed device work counter (fcs::launch_with_counter): rows take runs of frames from it
    // the build with L4 sums and the verdict launch (include/nstack_rxd.h); all null / 0 for the plain build
    uint32_t *dverdict;        // n words: the build's per-datagram accumulators, then the verdicts
    unsigned long long *bad;   // may be null
    uint32_t bad_mask;
    // include/nstack_gro.h: the build and the verdict launch of the coalescing forms (needs dverdict)
    uint32_t gro;
};

// The plan's scratch (device memory that lives on the stream between the launches).
struct Rec {   // the key record of a frame, written by the classify launch
    uint32_t src, dst;
    uint32_t w2;   // ip_id | ip_proto << 16 | MF << 24 | (hlen / 4) << 25 | groupable << 31
    uint32_t w3;   // o | L << 16 (RXR_WHOLE: I << 16)
};
struct Acc {   // what a group's fragments add up on the record of the frame that claimed (key, 0)
    unsigned long long sumL;
    uint32_t total, lasts, fault;
    uint32_t state;   // 0: not complete, 1: delivered, 2: too big (decide launch)
    uint32_t D, pad;
};
struct Entry {   // open addressing, keyed by (key, o) through the claimant's record
    uint32_t claim;   // frame index + 1; 0: empty
    uint32_t count;   // arrivals at this (key, o)
};
struct Scratch {
    Rec *rec;
    Acc *acc;
    uint32_t *headof;   // the frame that claimed (key, 0) of a fragment's group, or kNone32
    Entry *tab;
    uint64_t tsize;     // a power of two, >= 2 n
    uint64_t *totc, *totb;   // per-block totals of the two scans
};

constexpr int kThreads = 512;       // rxr_kernel: 8 waves per CU, a quarter-wave per frame
using plan::kPlanThreads;           // the plan kernels: one frame per thread
using plan::plan_blocks;
using plan::table_size;

// Bytes of scratch, and the carving of one allocation of that size (16-byte aligned parts).
inline uint64_t scratch_bytes(uint64_t n) {
    return n * (sizeof(Rec) + sizeof(Acc)) + table_size(n) * sizeof(Entry) + plan::up16(n * 4) + plan_blocks(n) * 16;
}
inline Scratch carve(void *mem, uint64_t n) {
    Scratch s;
    uint8_t *p = static_cast<uint8_t *>(mem);
    s.acc = reinterpret_cast<Acc *>(p);
    p += n * sizeof(Acc);
    s.tsize = table_size(n);
    s.tab = reinterpret_cast<Entry *>(p);
    p += s.tsize * sizeof(Entry);
    s.rec = reinterpret_cast<Rec *>(p);
    p += n * sizeof(Rec);
    s.headof = reinterpret_cast<uint32_t *>(p);
    p += plan::up16(n * 4);
    s.totc = reinterpret_cast<uint64_t *>(p);
    s.totb = s.totc + plan_blocks(n);
    return s;
}
// The part of the scratch the plan wants zeroed before its first launch: acc and the table (adjacent).
inline uint64_t zeroed_bytes(uint64_t n) { return n * sizeof(Acc) + table_size(n) * sizeof(Entry); }

enum class Route { kNone, kGeneral, kGeneralL4, kGro };
Route last_launch();      // what the last plain launch_build of this process launched (tests)
Route last_launch_l4();   // what the last launch_build with p.dverdict launched (tests)
Route last_launch_gro();  // what the last launch_build with p.gro launched (tests)

// The plan of p.n frames: the launches of include/nstack_rxr.h on `st`. `s` is carved scratch whose
// zeroed part has been zeroed on the stream.
hipError_t launch_plan(const RParams &p, const Scratch &s, hipStream_t st);

// Copies the delivered frames' bytes on a grid of at most `cus` workgroups; needs p.ctr. With
// p.dverdict (zeroed on the stream) the summing instantiation runs: every frame also adds the
// one's-complement sum of the bytes it stores to dverdict[dgi[i]]. With p.gro as well the coalescing
// instantiation runs (include/nstack_gro.h rule 4).
hipError_t launch_build(const RParams &p, int cus, hipStream_t st);

// The verdict word of every datagram k < min(counts[0], n) from dverdict[k] as launch_build left it
// and the delivered header in `out`; *bad (zeroed on the stream) counts verdict & bad_mask. With
// p.gro it is the finishing launch of include/nstack_gro.h: a merged datagram gets its TCP checksum.
hipError_t launch_verdict(const RParams &p, hipStream_t st);

}  // namespace rxr
