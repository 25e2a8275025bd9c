// mux_launch.hpp — host-side launchers of one-pass TX multiplexing (mux_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/nstack_mux.h"
#include "mux_plan.hpp"
#include "plan_prims.hpp"

namespace mux {

// What the kernels read and write (include/nstack_mux.h names every array).
struct MParams {
    uint64_t q, q_bytes;
    const uint64_t *rec;
    uint64_t n;
    const uint64_t *sfirst;
    const uint64_t *bind;
    const mux_tcb *tcb;         // may be null
    const mux_route *rt;
    const mux_neigh *nb;
    uint32_t S, R, N, id0, align;
    // the plan
    uint32_t *mstat;            // plan: out. build: the final word, may be null
    uint64_t *off;
    uint32_t *len;
    txf_l2 *l2;
    uint32_t *himg;             // ten dwords per record
    uint32_t *tnext;            // may be null
    uint64_t *counts;
    // the build
    const uint32_t *pstat;
    uint64_t dgram, dgram_bytes;
    unsigned long long *ctr;    // zeroed device work counter: rows take runs of records from it
};

constexpr int kThreads = 512;        // mux_kernel: a quarter-wave per record
using plan::kPlanThreads;            // the plan kernels
using plan::plan_blocks;
using plan::table_size;              // of the neighbour table: >= 2 N
using plan::up16;

// The plan's scratch (device memory that lives on the stream between the launches).
struct Scratch {
    unsigned long long *tkey;   // the neighbour table: tsize keys (0: empty; 1 << 32 | addr) ...
    uint32_t *tidx;             // ... and the lowest index that holds each
    uint64_t tsize;             // a power of two, >= 2 N
    uint32_t *sock;             // n: the record's socket, or kNone32
    uint32_t *rti, *nbi;        // n each: the route and the neighbour of a planned record
    uint32_t *pbytes;           // n: the padded size, then the sum of those in front inside the block
    uint32_t *ptcp;             // n: the TCP payload size, then the same prefix
    uint32_t *prank;            // n: the planned records in front inside the block
    uint64_t *totb;             // blocks + 1: the block totals of the padded sizes, then their scan; the last: the sum
    uint32_t *tott, *totr;      // blocks + 1 each: the same for the TCP payload and the planned count
};

// Bytes of scratch, and the carving of one allocation of that size (16-byte aligned parts). The parts
// the plan wants filled in front of its first launch lie first: the table keys (zero), then tidx
// (all ones).
inline uint64_t zero_bytes(uint64_t N) { return table_size(N) * 8; }
inline uint64_t ones_bytes(uint64_t N) { return up16(table_size(N) * 4); }
inline uint64_t scratch_bytes(uint64_t n, uint64_t N) {
    const uint64_t b = plan_blocks(n) + 1;
    return zero_bytes(N) + ones_bytes(N) + 6 * up16(n * 4) + up16(b * 8) + 2 * up16(b * 4);
}
// The bound include/nstack_mux.h states: 24 bytes of arrays and 16 / 256 of totals per n; 12 bytes per
// table entry, fewer than 4 N of them (or 16); nothing per S.
static_assert(kPlanThreads == 256, "kPlanThreads = 256 is behind the 1/16 of totals per n");
static_assert(MUX_SCRATCH_PER_N >= 24 + 1 && MUX_SCRATCH_PER_NB >= 4 * 12 && MUX_SCRATCH_FIXED >= 16 * 12 + 9 * 16 + 2 * 16,
              "the scratch bound of include/nstack_mux.h");
inline uint64_t scratch_bound(uint64_t n, uint64_t S, uint64_t N) {
    return n * MUX_SCRATCH_PER_N + S * MUX_SCRATCH_PER_S + N * MUX_SCRATCH_PER_NB + MUX_SCRATCH_FIXED;
}

inline Scratch carve(void *mem, uint64_t n, uint64_t N) {
    Scratch s;
    uint8_t *p = static_cast<uint8_t *>(mem);
    s.tsize = table_size(N);
    s.tkey = reinterpret_cast<unsigned long long *>(p);
    p += s.tsize * 8;
    s.tidx = reinterpret_cast<uint32_t *>(p);
    p += up16(s.tsize * 4);
    uint32_t **arr[] = {&s.sock, &s.rti, &s.nbi, &s.pbytes, &s.ptcp, &s.prank};
    for (uint32_t **a : arr) {
        *a = reinterpret_cast<uint32_t *>(p);
        p += up16(n * 4);
    }
    const uint64_t b = plan_blocks(n) + 1;
    s.totb = reinterpret_cast<uint64_t *>(p);
    p += up16(b * 8);
    s.tott = reinterpret_cast<uint32_t *>(p);
    p += up16(b * 4);
    s.totr = reinterpret_cast<uint32_t *>(p);
    return s;
}

enum class Route { kNone, kMux };
Route last_launch();   // what the last launch_build of this process launched (tests)

// The plan of p.n records on `st`. `s` is carved scratch whose first zero_bytes have been zeroed and
// next ones_bytes set to 0xff on the stream; p.counts has been zeroed on it.
hipError_t launch_plan(const MParams &p, const Scratch &s, hipStream_t st);

// Writes the datagrams on a grid of at most `cus` x 4 workgroups; needs p.ctr.
hipError_t launch_build(const MParams &p, int cus, hipStream_t st);

}  // namespace mux
