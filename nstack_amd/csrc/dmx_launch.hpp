// dmx_launch.hpp — host-side launchers of one-pass RX demultiplexing (dmx_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nstack_dmx.h"
#include "dmx_plan.hpp"
#include "plan_prims.hpp"

namespace dmx {

// What the kernels read and write (include/nstack_dmx.h names every array).
struct DParams {
    uint64_t out, out_bytes;
    const uint64_t *doff;
    const uint32_t *dlen;
    const uint32_t *dverdict;   // may be null
    const uint64_t *counts;
    uint64_t n;
    const uint64_t *bind;
    uint32_t S, drop_mask, align;
    // the plan
    uint32_t *dstat;            // plan: out. build: the final word, may be null
    uint32_t *dsock;
    uint64_t *rec;
    uint64_t *sbase;
    uint32_t *scnt;
    uint64_t *qcounts;
    // the build
    const uint32_t *pstat;
    uint64_t q, q_bytes;
    unsigned long long *ctr;    // zeroed device work counter: rows take runs of datagrams from it
};

constexpr int kThreads = 512;        // dmx_kernel: a quarter-wave per datagram
using plan::kPlanThreads;            // the plan kernels
using plan::plan_blocks;
using plan::table_size;              // of the bind table: >= 2 S
using plan::up16;
constexpr uint64_t kTile = 1024;     // elements of a partition tile: four rounds of kPlanThreads

// The plan's scratch (device memory that lives on the stream between the launches).
struct Scratch {
    unsigned long long *tkey;   // the bind table: tsize keys (0: empty) ...
    uint32_t *tidx;             // ... and the lowest index that holds each
    uint64_t tsize;             // a power of two, >= 2 S
    uint32_t *skey;             // n: the socket of a datagram with a record, else kNone32
    uint32_t *rsize;            // n: its record size
    uint32_t *key1, *key2;      // n each: the keys after the first and the second pass; kNone32 behind the records
    uint32_t *idx1, *idx2;      // n each: the datagram at each sorted position
    uint32_t *hist;             // 256 * tiles: (digit, tile) counts, then their exclusive scan
    uint64_t *tot;              // blocks: the block totals of the record sizes in sorted order, then their scan
};

inline uint64_t tiles(uint64_t n) { return (n + kTile - 1) / kTile; }
// Bytes of scratch, and the carving of one allocation of that size (16-byte aligned parts). The parts
// the plan wants filled in front of its first launch lie first: the table keys (zero), then tidx,
// key1 and key2 (all ones).
inline uint64_t zero_bytes(uint64_t S) { return table_size(S) * 8; }
inline uint64_t ones_bytes(uint64_t n, uint64_t S) { return up16(table_size(S) * 4) + 2 * up16(n * 4); }
inline uint64_t scratch_bytes(uint64_t n, uint64_t S) {
    return zero_bytes(S) + ones_bytes(n, S) + 4 * up16(n * 4) + up16(tiles(n) * 256 * 4) + up16(plan_blocks(n) * 8);
}
// The bound include/nstack_dmx.h states: 24 bytes of arrays, one of histogram and 1/32 of totals per
// n; 12 bytes per table entry, fewer than 4 S of them (or 16).
static_assert(kPlanThreads == 256, "kPlanThreads = 256 is behind the 1/32 of totals per n");
static_assert(DMX_SCRATCH_PER_N >= 24 + 1 + 1 && DMX_SCRATCH_PER_S >= 4 * 12 && DMX_SCRATCH_FIXED >= 16 * 12 + 9 * 16 + 1024 + 8,
              "the scratch bound of include/nstack_dmx.h");
inline uint64_t scratch_bound(uint64_t n, uint64_t S) { return n * DMX_SCRATCH_PER_N + S * DMX_SCRATCH_PER_S + DMX_SCRATCH_FIXED; }

inline Scratch carve(void *mem, uint64_t n, uint64_t S) {
    Scratch s;
    uint8_t *p = static_cast<uint8_t *>(mem);
    s.tsize = table_size(S);
    s.tkey = reinterpret_cast<unsigned long long *>(p);
    p += s.tsize * 8;
    s.tidx = reinterpret_cast<uint32_t *>(p);
    p += up16(s.tsize * 4);
    uint32_t **arr[] = {&s.key1, &s.key2, &s.skey, &s.rsize, &s.idx1, &s.idx2};
    for (uint32_t **a : arr) {
        *a = reinterpret_cast<uint32_t *>(p);
        p += up16(n * 4);
    }
    s.hist = reinterpret_cast<uint32_t *>(p);
    p += up16(tiles(n) * 256 * 4);
    s.tot = reinterpret_cast<uint64_t *>(p);
    return s;
}

enum class Route { kNone, kDemux };
Route last_launch();   // what the last launch_build of this process launched (tests)

// The plan of p.n datagrams on `st`. `s` is carved scratch whose first zero_bytes have been zeroed and
// next ones_bytes set to 0xff on the stream; p.qcounts has been zeroed on it.
hipError_t launch_plan(const DParams &p, const Scratch &s, hipStream_t st);

// Writes the records on a grid of at most `cus` workgroups; needs p.ctr.
hipError_t launch_build(const DParams &p, int cus, hipStream_t st);

}  // namespace dmx
