// txf_launch.hpp — host-side launchers of one-pass TX framing (txf_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plan_prims.hpp"
#include "tso_plan.hpp"
#include "txf_plan.hpp"

namespace txf {

// What both kernels read: datagram i = [dg + off[i], + len[i]); [lo4, hi4) is the readable range of
// the datagram arena, dword-rounded.
struct FParams {
    uint64_t dg;
    uint64_t lo4, hi4;
    const uint64_t *off;
    const uint32_t *len;
    uint64_t n;
    uint32_t mtu, flags;
    // frame building only
    const uint8_t *l2;       // 12-byte records
    const uint64_t *first;
    uint64_t out, slot, slots;
    uint32_t *flen, *status, *fcs;   // each may be null
    const uint32_t *blob;    // the FCS engine's constant tables (kFlagFcs only)
    unsigned long long *ctr; // zeroed device work counter (fcs::launch_with_counter): rows take runs of datagrams from it
    const uint16_t *mss;     // Mode::kTso only: per datagram (one with kFlagMssOne); may be null
};

// What a launch does with a datagram: the plain framer (nstack_txf.h), the framer that also fills the
// L4 checksums (nstack_txd.h), or that plus TCP segmentation (nstack_tso.h).
enum class Mode { kPlain, kL4, kTso };

constexpr int kThreads = 512;       // txf_kernel: 8 waves per CU, a quarter-wave per datagram
using plan::kPlanThreads;           // the plan kernels: one datagram per thread

enum class Route { kNone, kGeneral, kGeneralFcs, kGeneralL4, kGeneralL4Fcs, kTso, kTsoFcs };
Route last_launch();      // what the last launch_txf of Mode::kPlain of this process launched (tests)
Route last_launch_l4();   // the same for the launches of Mode::kL4
Route last_launch_tso();  // the same for the launches of Mode::kTso

// Builds the frames of p.n datagrams on a grid of at most `cus` workgroups; needs p.ctr. Mode::kL4:
// with the L4 checksum of every datagram (include/nstack_txd.h; p.flags may hold kFlagUdpZero);
// Mode::kTso: that, and eligible TCP datagrams cut into MSS segments (include/nstack_tso.h; p.mss).
hipError_t launch_txf(const FParams &p, Mode mode, int cus, hipStream_t st);

// status[i] (may be null) and first[0..n]: counts and per-block totals, the scan of the totals in
// one workgroup, the add; three launches on `st`. tot holds ceil(n / kPlanThreads) u64 of scratch.
hipError_t launch_plan(const FParams &p, uint32_t *status, uint64_t *first, uint64_t *tot, hipStream_t st);

// The same for include/nstack_tso.h (p.mss; status[i] the whole word without TXF_NO_ROOM): its own
// count kernel, then the two scan launches of launch_plan.
hipError_t launch_plan_tso(const FParams &p, uint32_t *status, uint64_t *first, uint64_t *tot, hipStream_t st);

}  // namespace txf
