// rxv_launch.hpp — host-side launcher of the one-pass RX validator (rxv_kernel.hip), and the
// routing band, grid sizes and eight-way dispatch it shares with the sealer's (txs_launch.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fcs_launch.hpp"

namespace rxv {

// Verdict bits and flags (include/nstack_rxv.h).
constexpr uint32_t kFcsBad = 0x001u, kRunt = 0x002u, kIpv4 = 0x004u, kIpBadHdr = 0x008u, kIpBadLen = 0x010u,
                   kIpBadCsum = 0x020u, kFrag = 0x040u, kL4Checked = 0x080u, kL4BadCsum = 0x100u,
                   kL4Short = 0x200u;
constexpr int kProtoShift = 16;
constexpr uint32_t kFlagTrailer = 1u;

struct RParams {
    uint64_t base;          // fixed: frame 0 start; var: arena start
    uint64_t stride;        // fixed only
    const uint64_t *off;    // var only
    const uint32_t *len;    // var only
    uint32_t *verdict;
    unsigned long long *bad;   // null: no count
    uint64_t n;
    uint64_t lo4, hi4;      // readable byte range, dword-rounded
    uint32_t flen;          // fixed: frame length
    uint32_t bad_mask;
    unsigned long long *ctr;   // rxv_dma_kernel: zeroed device work counter (fcs::launch_with_counter)
    uint32_t zmax;          // max leading bytes a front lane masks (fcs::KParams::zmax; 96 for variable batches)
    const uint32_t *blob;   // the FCS engine's constant tables (fcs::kBlobWords)
};

// rxv_kernel: 8 waves per CU. 16 waves need 128 VGPRs or fewer, which the kernel with the CRC
// (about 150) does not reach without spilling.
constexpr int kThreads = 512;

// One quarter-wave per frame (rxv_kernel<VAR, TRAILER, TINY, kThreads>) on a grid of at most `cus`
// workgroups; tiny = fcs::fixed_tiny's bound.
constexpr int kDmaThreads = 1024;   // rxv_dma_kernel: 16 waves per CU, one 6 KiB LDS slot each

// The kernel launch_rxv takes: kDma = rxv_dma_kernel (fixed strides of more than dma_min frames of
// 1496..1524 B whose four-frame items fit a slot: fcs::fixed_dma; the only one that needs p.ctr),
// kGeneral = rxv_kernel (every other shape), kNone (n == 0). Verdicts are identical either way.
enum class Route { kNone, kGeneral, kDma };
Route route(bool var, const RParams &p, uint64_t dma_min);

// The routing both directions share (rxv::route is this; txs::route adds its stride condition).
inline Route dma_band_route(bool var, const RParams &p, uint64_t dma_min) {
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

// Grids of at most `cus` workgroups, one per CU: the LDS-DMA kernels' (16 waves of four-frame
// items) and the quarter-wave kernels' (persistent over the frames, a quarter-wave per frame).
inline int dma_grid(uint64_t n, int cus) {
    const uint64_t items = (n + 3) / 4, want = (items + kDmaThreads / 64 - 1) / (kDmaThreads / 64);
    return (int)(want < (uint64_t)cus ? want : (uint64_t)cus);
}
inline int walk_grid(uint64_t n, int cus) {
    const uint64_t slots = kThreads / fcs::kGroup, want = (n + slots - 1) / slots;
    return (int)(want < (uint64_t)cus ? want : (uint64_t)cus);
}
inline bool walk_tiny(const RParams &p) { return p.hi4 - p.lo4 < 2 * (uint64_t)fcs::kChunkBytes; }

// Launches KERNEL<var, x, tiny, kThreads>(arg), one of its eight instantiations, from run-time bools.
#define FRAME_WALK_GO(KERNEL, V, X, S, grid, st, arg) \
    hipLaunchKernelGGL((KERNEL<V, X, S, kThreads>), dim3(grid), dim3(kThreads), 0, st, arg)
#define FRAME_WALK_GO2(KERNEL, V, X, tiny, grid, st, arg)                   \
    do {                                                                     \
        if (tiny) FRAME_WALK_GO(KERNEL, V, X, true, grid, st, arg);          \
        else FRAME_WALK_GO(KERNEL, V, X, false, grid, st, arg);              \
    } while (0)
#define FRAME_WALK_LAUNCH(KERNEL, var, x, tiny, grid, st, arg)               \
    do {                                                                     \
        if (var) {                                                           \
            if (x) FRAME_WALK_GO2(KERNEL, true, true, tiny, grid, st, arg);  \
            else FRAME_WALK_GO2(KERNEL, true, false, tiny, grid, st, arg);   \
        } else {                                                             \
            if (x) FRAME_WALK_GO2(KERNEL, false, true, tiny, grid, st, arg); \
            else FRAME_WALK_GO2(KERNEL, false, false, tiny, grid, st, arg);  \
        }                                                                    \
    } while (0)

Route last_launch();   // what the last launch_rxv of this process launched (tests)
hipError_t launch_rxv(bool var, bool trailer, const RParams &p, int cus, uint64_t dma_min, hipStream_t st);

}  // namespace rxv
