// rxv_engine.cpp — the C ABI of include/nstack_rxv.h around rxv_kernel.hip.
//
// Device forms validate and launch; the host form runs a double-buffered H2D -> kernel -> D2H
// pipeline of 64 MiB chunks on the engine's first GPU, in staging of its own (as inet_engine.cpp's
// run_host: frames of a chunk are copied as one span when they lie densely, gathered otherwise).
// No CPU path: a failure is returned, never answered on the host, and the FCS engine's host-batch
// and fallback counters are not touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "../../include/nstack_rxv.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "rxv_launch.hpp"

namespace {

int hip_fail(hipError_t e, const char *what) {
    const int err = (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu ||
                     e == hipErrorInvalidDeviceFunction || e == hipErrorInvalidImage)
                        ? ENODEV
                        : (e == hipErrorOutOfMemory ? ENOMEM : EIO);
    return fcs::set_error(err, "%s: %s", what, hipGetErrorString(e));
}

#define HIPTRY(expr, what)                                 \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return hip_fail(e_, what);   \
    } while (0)

inline uint64_t floor4(uint64_t x) { return x & ~3ull; }
inline uint64_t ceil4(uint64_t x) { return (x + 3) & ~3ull; }

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

int copy_name(const char *r, char *out, uint64_t cap) {
    if (!out || cap == 0) return -EINVAL;
    const uint64_t k = std::min<uint64_t>(std::strlen(r), cap - 1);
    std::memcpy(out, r, k);
    out[k] = 0;
    return (int)k;
}

// ---- host pipeline ----
constexpr uint64_t kChunkBytes = 64ull << 20;
constexpr uint64_t kChunkPkts = 1ull << 20;
constexpr int kDepth = 2;

struct Slot {
    uint8_t *d_in = nullptr, *h_in = nullptr;
    uint64_t *d_off = nullptr, *h_off = nullptr;
    uint32_t *d_len = nullptr, *h_len = nullptr;
    uint32_t *d_out = nullptr, *h_out = nullptr;   // the chunk's verdicts, then its bad count (u64)
    hipEvent_t done = nullptr;
    bool live = false;
    uint64_t i0 = 0, n = 0;
};

struct HostPipe {
    std::mutex mu;
    int dev = -1, cus = 0;
    hipStream_t stream = nullptr;
    Slot slot[kDepth];
};

std::mutex g_pipes_mu;
std::map<int, std::unique_ptr<HostPipe>> g_pipes;

void free_pipe(HostPipe &hp) {
    for (Slot &s : hp.slot) {
        if (s.done) (void)hipEventDestroy(s.done);
        for (void *d : {(void *)s.d_in, (void *)s.d_off, (void *)s.d_len, (void *)s.d_out})
            if (d) (void)hipFree(d);
        for (void *h : {(void *)s.h_in, (void *)s.h_off, (void *)s.h_len, (void *)s.h_out})
            if (h) (void)hipHostFree(h);
        s = Slot{};
    }
    if (hp.stream) (void)hipStreamDestroy(hp.stream);
    hp.stream = nullptr;
}

int alloc_pipe(HostPipe &hp) {
    HIPTRY(hipSetDevice(hp.dev), "hipSetDevice");
    HIPTRY(hipStreamCreateWithFlags(&hp.stream, hipStreamNonBlocking), "hipStreamCreate");
    for (Slot &s : hp.slot) {
        HIPTRY(hipMalloc(&s.d_in, kChunkBytes + 64), "hipMalloc(rxv staging)");
        HIPTRY(hipHostMalloc(&s.h_in, kChunkBytes + 64, hipHostMallocDefault), "hipHostMalloc(rxv staging)");
        HIPTRY(hipMalloc(&s.d_off, kChunkPkts * 8), "hipMalloc(off)");
        HIPTRY(hipHostMalloc(&s.h_off, kChunkPkts * 8, hipHostMallocDefault), "hipHostMalloc(off)");
        HIPTRY(hipMalloc(&s.d_len, kChunkPkts * 4), "hipMalloc(len)");
        HIPTRY(hipHostMalloc(&s.h_len, kChunkPkts * 4, hipHostMallocDefault), "hipHostMalloc(len)");
        HIPTRY(hipMalloc(&s.d_out, kChunkPkts * 4 + 8), "hipMalloc(verdict)");
        HIPTRY(hipHostMalloc(&s.h_out, kChunkPkts * 4 + 8, hipHostMallocDefault), "hipHostMalloc(verdict)");
        HIPTRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate");
    }
    return 0;
}

int get_pipe(int dev, int cus, HostPipe **out) {
    std::lock_guard<std::mutex> lk(g_pipes_mu);
    auto &up = g_pipes[dev];
    if (!up) {
        auto hp = std::make_unique<HostPipe>();
        hp->dev = dev;
        hp->cus = cus;
        const int rc = alloc_pipe(*hp);
        if (rc) {   // a half-built pipeline holds nothing: the next call starts over
            free_pipe(*hp);
            return rc;
        }
        up = std::move(hp);
    }
    *out = up.get();
    return 0;
}

int64_t run_host(const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t flags, uint32_t bad_mask,
                 uint32_t *verdict, uint64_t n) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    HostPipe *hp = nullptr;
    if ((rc = get_pipe(dev, cus, &hp))) return rc;
    std::lock_guard<std::mutex> lk(hp->mu);
    int cur = 0;
    HIPTRY(hipGetDevice(&cur), "hipGetDevice");
    HIPTRY(hipSetDevice(dev), "hipSetDevice");
    uint64_t bad = 0;
    auto drain = [&](Slot &s) -> int {
        if (!s.live) return 0;
        HIPTRY(hipEventSynchronize(s.done), "hipEventSynchronize");
        std::memcpy(verdict + s.i0, s.h_out, s.n * 4);
        uint64_t b = 0;
        std::memcpy(&b, s.h_out + kChunkPkts, 8);
        bad += b;
        s.live = false;
        return 0;
    };
    uint64_t i = 0;
    int b = 0;
    auto step = [&]() -> int {
        Slot &s = hp->slot[b];
        int rc = drain(s);
        if (rc) return rc;
        // the chunk [i, e): as inet_engine.cpp's run_host
        uint64_t e = i, sum = 0, lo = UINT64_MAX, hi = 0;
        while (e < n && e - i < kChunkPkts && sum + len[e] <= kChunkBytes) {
            const uint64_t nlo = std::min(lo, off[e]), nhi = std::max(hi, off[e] + len[e]);
            if (e > i && nhi - nlo > kChunkBytes && nhi - nlo <= 2 * (sum + len[e])) break;
            sum += len[e];
            lo = nlo;
            hi = nhi;
            e++;
        }
        if (e == i)
            return fcs::set_error(EINVAL, "frame %llu of %u bytes exceeds the %llu-byte host chunk",
                                  (unsigned long long)i, len[i], (unsigned long long)kChunkBytes);
        const uint64_t np = e - i;
        uint64_t span;
        if (hi - lo <= kChunkBytes) {   // dense: one span copy, offsets rebased (alignment kept mod 16)
            const uint64_t pad = lo & 15;
            span = pad + (hi - lo);
            fcs::staging_copy(s.h_in + pad, arena + lo, hi - lo);
            for (uint64_t q = 0; q < np; q++) s.h_off[q] = off[i + q] - lo + pad;
        } else {                        // sparse: gather back to back
            uint64_t w = 0;
            for (uint64_t q = 0; q < np; q++) {
                std::memcpy(s.h_in + w, arena + off[i + q], len[i + q]);
                s.h_off[q] = w;
                w += len[i + q];
            }
            span = w;
        }
        std::memcpy(s.h_len, len + i, np * 4);
        hipStream_t st = hp->stream;
        if (span) HIPTRY(hipMemcpyAsync(s.d_in, s.h_in, span, hipMemcpyHostToDevice, st), "H2D frames");
        HIPTRY(hipMemcpyAsync(s.d_off, s.h_off, np * 8, hipMemcpyHostToDevice, st), "H2D off");
        HIPTRY(hipMemcpyAsync(s.d_len, s.h_len, np * 4, hipMemcpyHostToDevice, st), "H2D len");
        HIPTRY(hipMemsetAsync(s.d_out + kChunkPkts, 0, 8, st), "zeroing bad count");
        rxv::RParams p{};
        p.base = (uint64_t)s.d_in;
        p.off = s.d_off;
        p.len = s.d_len;
        p.verdict = s.d_out;
        p.bad = (unsigned long long *)(s.d_out + kChunkPkts);
        p.n = np;
        p.lo4 = floor4(p.base);
        p.hi4 = ceil4(p.base + kChunkBytes + 64);   // the staging buffer: always more than two lane chunks
        p.bad_mask = bad_mask;
        p.zmax = 96;
        if ((rc = launch(true, p, flags, hp->dev, cus, st))) return rc;
        if (np < kChunkPkts) {
            HIPTRY(hipMemcpyAsync(s.h_out, s.d_out, np * 4, hipMemcpyDeviceToHost, st), "D2H verdicts");
            HIPTRY(hipMemcpyAsync(s.h_out + kChunkPkts, s.d_out + kChunkPkts, 8, hipMemcpyDeviceToHost, st), "D2H bad count");
        } else {
            HIPTRY(hipMemcpyAsync(s.h_out, s.d_out, np * 4 + 8, hipMemcpyDeviceToHost, st), "D2H verdicts");
        }
        HIPTRY(hipEventRecord(s.done, st), "hipEventRecord");
        s.live = true;
        s.i0 = i;
        s.n = np;
        i = e;
        b = (b + 1) % kDepth;
        return 0;
    };
    while (i < n && !rc) rc = step();
    if (rc) {   // never leave a slot that would later be drained into this call's verdicts
        (void)hipStreamSynchronize(hp->stream);
        for (Slot &s : hp->slot) s.live = false;
    }
    for (Slot &s : hp->slot) {
        const int r2 = drain(s);
        if (!rc) rc = r2;
    }
    hipSetDevice(cur);
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
    rxv::RParams p{};
    p.base = (uint64_t)arena;
    p.off = off;
    p.len = len;
    p.verdict = verdict;
    p.bad = (unsigned long long *)bad;
    p.n = n;
    p.lo4 = floor4(p.base);
    p.hi4 = ceil4(p.base + arena_bytes);
    p.bad_mask = bad_mask;
    p.zmax = 96;
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
    rxv::RParams p{};
    p.base = (uint64_t)base;
    p.stride = stride;
    p.flen = len;
    p.verdict = verdict;
    p.bad = (unsigned long long *)bad;
    p.n = n;
    p.lo4 = floor4(p.base);
    p.hi4 = ceil4(p.base + (n - 1) * stride + len);
    p.bad_mask = bad_mask;
    p.zmax = fcs::mask_bound(len);
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
    rxv::RParams p{};
    p.base = base;
    p.stride = stride;
    p.flen = len;
    p.n = n;
    p.lo4 = floor4(base);
    p.hi4 = n ? ceil4(base + (n - 1) * stride + len) : p.lo4;
    return copy_name(route_name(rxv::route(false, p, g_dma_min.load(std::memory_order_relaxed))), out, cap);
}

// The kernel the last ether_rx_validate launch of this process actually launched.
int fcs_debug_rxv_last_launch(char *out, uint64_t cap) { return copy_name(route_name(rxv::last_launch()), out, cap); }

}  // extern "C"
