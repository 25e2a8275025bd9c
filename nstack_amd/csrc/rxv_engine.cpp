// rxv_engine.cpp — the C ABI of include/nstack_rxv.h around rxv_kernel.hip.
//
// Device forms validate and launch; the host form runs the double-buffered H2D -> kernel -> D2H
// pipeline of host_pipe.hpp in 64 MiB chunks on the engine's first GPU, in staging of its own, cut
// and staged by host_chunk.hpp (frames of a chunk are copied as one span when they lie densely,
// gathered otherwise). No CPU path: a failure is returned, never answered on the host, and the FCS
// engine's host-batch and fallback counters are not touched.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <cstring>

#include "../../include/nstack_rxv.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_pipe.hpp"
#include "rxv_launch.hpp"

using namespace hostpipe;

namespace {

int check_flags(uint32_t flags) {
    if (flags & ~RXV_F_TRAILER) return fcs::set_error(EINVAL, "unknown flag bits 0x%x", flags & ~RXV_F_TRAILER);
    return 0;
}

std::atomic<uint64_t> g_dma_min{16384};   // see ether_rx_validate_set_dma_threshold

// launch_rxv with the work counter the LDS-DMA route takes (the same rxv::route decision the
// launcher makes), leased from the FCS engine's ring of device `dev` for this launch.
int launch(bool var, rxv::RParams &p, uint32_t flags, int dev, int cus, hipStream_t st) {
    int rc = fcs::device_tables(dev, &p.blob);
    if (rc) return rc;
    const uint64_t dma_min = g_dma_min.load(std::memory_order_relaxed);
    auto go = [&](unsigned long long *ctr) -> int {
        p.ctr = ctr;
        HIPTRY(rxv::launch_rxv(var, (flags & RXV_F_TRAILER) != 0, p, cus, dma_min, st), "launching the rxv kernel");
        return 0;
    };
    if (rxv::route(var, p, dma_min) == rxv::Route::kDma) return fcs::launch_with_counter(dev, (void *)st, go);
    return go(nullptr);
}

const char *route_name(rxv::Route r) {
    return r == rxv::Route::kDma ? "lds-dma" : (r == rxv::Route::kGeneral ? "general" : "none");
}

// The parameters of a variable batch whose frames lie in the `bytes` bytes at `base`.
rxv::RParams var_params(uint64_t base, uint64_t bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                        uint32_t bad_mask, uint32_t *verdict, void *bad) {
    rxv::RParams p{};
    p.base = base;
    p.off = off;
    p.len = len;
    p.verdict = verdict;
    p.bad = (unsigned long long *)bad;
    p.n = n;
    p.lo4 = floor4(base);
    p.hi4 = ceil4(base + bytes);
    p.bad_mask = bad_mask;
    p.zmax = 96;
    return p;
}

// The parameters of a fixed-stride batch: what the launch gets and what fcs_debug_rxv_route names.
rxv::RParams fixed_params(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, uint32_t bad_mask,
                          uint32_t *verdict, void *bad) {
    rxv::RParams p{};
    p.base = base;
    p.stride = stride;
    p.flen = len;
    p.verdict = verdict;
    p.bad = (unsigned long long *)bad;
    p.n = n;
    p.lo4 = floor4(base);
    p.hi4 = n ? ceil4(base + (n - 1) * stride + len) : p.lo4;
    p.bad_mask = bad_mask;
    p.zmax = fcs::mask_bound(len);
    return p;
}

// ---- host pipeline ----
constexpr uint64_t kChunkBytes = 64ull << 20;
constexpr uint64_t kChunkPkts = 1ull << 20;
constexpr int kDepth = 2;

struct RxvPipe;                   // names this engine's pipelines (host_pipe.hpp)
enum { kIn, kOff, kLen, kOut };   // kOut: the chunk's verdicts, then its bad count (u64)
const std::vector<BufSpec> kBufs = {{kChunkBytes + 64, "rxv staging"}, {kChunkPkts * 8, "off"},
                                    {kChunkPkts * 4, "len"},           {kChunkPkts * 4 + 8, "verdict"}};

int64_t run_host(const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t flags, uint32_t bad_mask,
                 uint32_t *verdict, uint64_t n) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    uint64_t bad = 0;
    auto issue = [&](Slot &s, hipStream_t st, uint64_t i) -> int64_t {
        const hostchunk::Cut c = hostchunk::cut(off, len, i, n, kChunkBytes, kChunkPkts, 0);
        if (c.e == i)
            return fcs::set_error(EINVAL, "frame %llu of %u bytes exceeds the %llu-byte host chunk",
                                  (unsigned long long)i, len[i], (unsigned long long)kChunkBytes);
        const uint64_t np = c.e - i;
        int rc = stage_h2d(s, st, arena, off, len, i, c, kChunkBytes, 0, "H2D frames");
        if (rc) return rc;
        uint32_t *d_out = s.d<uint32_t>(kOut), *h_out = s.h<uint32_t>(kOut);
        HIPTRY(hipMemsetAsync(d_out + kChunkPkts, 0, 8, st), "zeroing bad count");
        // the arena is the staging buffer: always more than two lane chunks
        rxv::RParams p = var_params((uint64_t)s.d<void>(kIn), kChunkBytes + 64, s.d<uint64_t>(kOff),
                                    s.d<uint32_t>(kLen), np, bad_mask, d_out, d_out + kChunkPkts);
        if ((rc = launch(true, p, flags, dev, cus, st))) return rc;
        HIPTRY(hipMemcpyAsync(h_out, d_out, np * 4, hipMemcpyDeviceToHost, st), "D2H verdicts");
        HIPTRY(hipMemcpyAsync(h_out + kChunkPkts, d_out + kChunkPkts, 8, hipMemcpyDeviceToHost, st), "D2H bad count");
        s.i0 = i;
        s.n = np;
        s.live = true;
        return (int64_t)c.e;
    };
    auto drain = [&](Slot &s) {
        std::memcpy(verdict + s.i0, s.h<uint32_t>(kOut), s.n * 4);
        uint64_t b = 0;
        std::memcpy(&b, s.h<uint32_t>(kOut) + kChunkPkts, 8);
        bad += b;
    };
    rc = run_pipe<RxvPipe>(dev, kDepth, kBufs, n, issue, drain);
    return rc ? (int64_t)rc : (int64_t)bad;
}

}  // namespace

extern "C" {

int ether_rx_validate_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                          uint32_t flags, uint32_t bad_mask, uint32_t *verdict, uint64_t *bad, uint64_t n,
                          void *stream) {
    int rc = check_flags(flags);
    if (rc) return rc;
    if (n && !verdict) return fcs::set_error(EINVAL, "null verdict array");
    if (n && (!arena || !off || !len)) return fcs::set_error(EINVAL, "null pointer");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (bad) HIPTRY(hipMemsetAsync(bad, 0, 8, (hipStream_t)stream), "zeroing bad count");
    if (n == 0) return 0;
    rxv::RParams p = var_params((uint64_t)arena, arena_bytes, off, len, n, bad_mask, verdict, bad);
    return launch(true, p, flags, dev, cus, (hipStream_t)stream);
}

int ether_rx_validate_fixed_dev(const void *base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags,
                                uint32_t bad_mask, uint32_t *verdict, uint64_t *bad, void *stream) {
    int rc = check_flags(flags);
    if (rc) return rc;
    if (n && !verdict) return fcs::set_error(EINVAL, "null verdict array");
    if (n && !base) return fcs::set_error(EINVAL, "null pointer");
    if (n > 1 && stride < len) return fcs::set_error(EINVAL, "stride %llu < len %u", (unsigned long long)stride, len);
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (bad) HIPTRY(hipMemsetAsync(bad, 0, 8, (hipStream_t)stream), "zeroing bad count");
    if (n == 0) return 0;
    rxv::RParams p = fixed_params((uint64_t)base, stride, len, n, bad_mask, verdict, bad);
    return launch(false, p, flags, dev, cus, (hipStream_t)stream);
}

int64_t ether_rx_validate_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                               uint32_t flags, uint32_t bad_mask, uint32_t *verdict, uint64_t n) {
    const int rc = check_flags(flags);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!verdict) return fcs::set_error(EINVAL, "null verdict array");
    if (!arena || !off || !len) return fcs::set_error(EINVAL, "null pointer");
    for (uint64_t i = 0; i < n; i++)
        if (off[i] > arena_bytes || len[i] > arena_bytes - off[i])
            return fcs::set_error(EINVAL, "frame %llu [%llu, +%u) outside the %llu-byte arena",
                                  (unsigned long long)i, (unsigned long long)off[i], len[i],
                                  (unsigned long long)arena_bytes);
    return run_host((const uint8_t *)arena, off, len, flags, bad_mask, verdict, n);
}

uint64_t ether_rx_validate_set_dma_threshold(uint64_t frames) { return g_dma_min.exchange(frames); }

// rxv::route's decision for a fixed-stride batch, named (no device call).
int fcs_debug_rxv_route(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, char *out, uint64_t cap) {
    const rxv::RParams p = fixed_params(base, stride, len, n, 0, nullptr, nullptr);
    return copy_name(route_name(rxv::route(false, p, g_dma_min.load(std::memory_order_relaxed))), out, cap);
}

// The kernel the last ether_rx_validate launch of this process actually launched.
int fcs_debug_rxv_last_launch(char *out, uint64_t cap) { return copy_name(route_name(rxv::last_launch()), out, cap); }

}  // extern "C"
