// txs_launch.hpp — host-side launcher of one-pass TX sealing (txs_kernel.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "rxv_launch.hpp"

namespace txs {

// Status bits and flags (include/nstack_txs.h). Runt, IPv4, bad header, bad length, fragment and
// short L4 are the validator's bits (rxv_launch.hpp), so the status word is assembled as a verdict is.
constexpr uint32_t kFcsSet = 0x001u, kRunt = rxv::kRunt, kIpv4 = rxv::kIpv4, kIpBadHdr = rxv::kIpBadHdr,
                   kIpBadLen = rxv::kIpBadLen, kIpCsumSet = 0x020u, kFrag = rxv::kFrag, kL4CsumSet = 0x080u,
                   kL4Short = rxv::kL4Short;
constexpr int kProtoShift = rxv::kProtoShift;
constexpr uint32_t kFlagFcs = 1u, kFlagUdpZero = 2u;

struct Fields {   // struct txs_fields
    uint16_t ip_csum, l4_csum;
    uint32_t fcs;
};

// The validator's geometry (base, stride / off, len, n, lo4, hi4, flen, zmax, blob, ctr) with
// r.verdict = the status words (may be null here), r.bad = the count, r.bad_mask = the count mask.
// base and [lo4, hi4) are written to: hi4 includes the last FCS place with kFlagFcs.
struct TParams {
    rxv::RParams r;
    Fields *fields;   // may be null
    uint32_t flags;
};

constexpr int kThreads = rxv::kThreads;         // txs_kernel: 8 waves per CU, as rxv_kernel
constexpr int kDmaThreads = rxv::kDmaThreads;   // txs_dma_kernel: 16 waves per CU, one 6 KiB LDS slot each

// The kernel launch_txs takes: kDma = txs_dma_kernel (fixed strides of more than dma_min frames in
// fcs::fixed_dma's band; with kFlagFcs the stride must also hold the FCS place: stride >= len + 4;
// the only one that needs p.r.ctr), kGeneral = txs_kernel (every other shape), kNone (n == 0). The
// bytes written are identical either way.
using Route = rxv::Route;
Route route(bool var, const TParams &p, uint64_t dma_min);
Route last_launch();   // what the last launch_txs of this process launched (tests)
hipError_t launch_txs(bool var, const TParams &p, int cus, uint64_t dma_min, hipStream_t st);

}  // namespace txs
