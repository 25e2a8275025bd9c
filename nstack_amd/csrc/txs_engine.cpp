// txs_engine.cpp — the C ABI of include/nstack_txs.h around txs_kernel.hip.
//
// Device forms validate and launch; the host form runs a double-buffered H2D -> kernel -> D2H
// pipeline of 64 MiB chunks on the engine's first GPU, in staging of its own (as rxv_engine.cpp's
// run_host). Only the status word and the 8-byte fields record of each frame travel back: the
// caller's frames are patched from them on the host (where to write follows from the status bits
// and the header), the frame bytes do not travel back. No CPU path: a failure is returned, never
// answered on the host, and the FCS engine's host-batch and fallback counters are not touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>

#include "../../include/nstack_txs.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "txs_launch.hpp"

static_assert(sizeof(txs_fields) == 8 && sizeof(txs::Fields) == 8, "the fields record is 8 bytes");

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
    const uint32_t known = TXS_F_FCS | TXS_F_UDP_ZERO;
    if (flags & ~known) return fcs::set_error(EINVAL, "unknown flag bits 0x%x", flags & ~known);
    return 0;
}

std::atomic<uint64_t> g_dma_min{16384};   // see ether_tx_seal_set_dma_threshold

// launch_txs with the work counter the LDS-DMA route takes (the same txs::route decision the
// launcher makes), leased from the FCS engine's ring of device `dev` for this launch.
int launch(bool var, txs::TParams &tp, int dev, int cus, hipStream_t st) {
    int rc = fcs::device_tables(dev, &tp.r.blob);
    if (rc) return rc;
    const uint64_t dma_min = g_dma_min.load(std::memory_order_relaxed);
    auto go = [&](unsigned long long *ctr) -> int {
        tp.r.ctr = ctr;
        HIPTRY(txs::launch_txs(var, tp, cus, dma_min, st), "launching the txs kernel");
        return 0;
    };
    if (txs::route(var, tp, dma_min) == txs::Route::kDma) return fcs::launch_with_counter(dev, (void *)st, go);
    return go(nullptr);
}

const char *route_name(txs::Route r) {
    return r == txs::Route::kDma ? "lds-dma" : (r == txs::Route::kGeneral ? "general" : "none");
}

int copy_name(const char *r, char *out, uint64_t cap) {
    if (!out || cap == 0) return -EINVAL;
    const uint64_t k = std::min<uint64_t>(std::strlen(r), cap - 1);
    std::memcpy(out, r, k);
    out[k] = 0;
    return (int)k;
}

// What the device wrote into a frame, repeated on the caller's host copy of it.
void patch_host(uint8_t *fr, uint32_t len, uint32_t flags, uint32_t status, const txs::Fields &fl) {
    if (status & TXS_IP_CSUM_SET) {
        std::memcpy(fr + 24, &fl.ip_csum, 2);
        const uint32_t proto = (status >> TXS_PROTO_SHIFT) & 0xffu, l4 = 14u + (fr[14] & 0x0fu) * 4u;
        const bool udp_zero = (flags & TXS_F_UDP_ZERO) && proto == 17u &&
                              !(status & (TXS_IP_BAD_LEN | TXS_FRAG | TXS_L4_SHORT));
        if ((status & TXS_L4_CSUM_SET) || udp_zero)
            std::memcpy(fr + l4 + (proto == 6u ? 16u : (proto == 17u ? 6u : 2u)), &fl.l4_csum, 2);
    }
    if (status & TXS_FCS_SET) {
        const uint8_t b[4] = {(uint8_t)fl.fcs, (uint8_t)(fl.fcs >> 8), (uint8_t)(fl.fcs >> 16), (uint8_t)(fl.fcs >> 24)};
        std::memcpy(fr + len, b, 4);
    }
}

// ---- host pipeline ----
constexpr uint64_t kChunkBytes = 64ull << 20;
constexpr uint64_t kChunkPkts = 1ull << 20;
constexpr int kDepth = 2;
// a chunk's results: status words, the count (u64), the fields records
constexpr uint64_t kOutCount = kChunkPkts * 4, kOutFields = kOutCount + 8, kOutBytes = kOutFields + kChunkPkts * 8;

struct Slot {
    uint8_t *d_in = nullptr, *h_in = nullptr;
    uint64_t *d_off = nullptr, *h_off = nullptr;
    uint32_t *d_len = nullptr, *h_len = nullptr;
    uint8_t *d_out = nullptr, *h_out = nullptr;
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
        HIPTRY(hipMalloc(&s.d_in, kChunkBytes + 64), "hipMalloc(txs staging)");
        HIPTRY(hipHostMalloc(&s.h_in, kChunkBytes + 64, hipHostMallocDefault), "hipHostMalloc(txs staging)");
        HIPTRY(hipMalloc(&s.d_off, kChunkPkts * 8), "hipMalloc(off)");
        HIPTRY(hipHostMalloc(&s.h_off, kChunkPkts * 8, hipHostMallocDefault), "hipHostMalloc(off)");
        HIPTRY(hipMalloc(&s.d_len, kChunkPkts * 4), "hipMalloc(len)");
        HIPTRY(hipHostMalloc(&s.h_len, kChunkPkts * 4, hipHostMallocDefault), "hipHostMalloc(len)");
        HIPTRY(hipMalloc(&s.d_out, kOutBytes), "hipMalloc(status)");
        HIPTRY(hipHostMalloc(&s.h_out, kOutBytes, hipHostMallocDefault), "hipHostMalloc(status)");
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

int64_t run_host(uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t flags, uint32_t count_mask,
                 uint32_t *status, uint64_t n) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    HostPipe *hp = nullptr;
    if ((rc = get_pipe(dev, cus, &hp))) return rc;
    std::lock_guard<std::mutex> lk(hp->mu);
    int cur = 0;
    HIPTRY(hipGetDevice(&cur), "hipGetDevice");
    HIPTRY(hipSetDevice(dev), "hipSetDevice");
    const uint64_t T = (flags & TXS_F_FCS) ? 4 : 0;   // bytes behind each frame that belong to it
    uint64_t count = 0;
    auto drain = [&](Slot &s) -> int {
        if (!s.live) return 0;
        HIPTRY(hipEventSynchronize(s.done), "hipEventSynchronize");
        const uint32_t *st = reinterpret_cast<const uint32_t *>(s.h_out);
        const txs::Fields *fl = reinterpret_cast<const txs::Fields *>(s.h_out + kOutFields);
        for (uint64_t q = 0; q < s.n; q++) patch_host(arena + off[s.i0 + q], len[s.i0 + q], flags, st[q], fl[q]);
        if (status) std::memcpy(status + s.i0, st, s.n * 4);
        uint64_t b = 0;
        std::memcpy(&b, s.h_out + kOutCount, 8);
        count += b;
        s.live = false;
        return 0;
    };
    uint64_t i = 0;
    int b = 0;
    auto step = [&]() -> int {
        Slot &s = hp->slot[b];
        int rc = drain(s);
        if (rc) return rc;
        // the chunk [i, e): as rxv_engine.cpp's run_host, every frame with its FCS place
        uint64_t e = i, sum = 0, lo = UINT64_MAX, hi = 0;
        while (e < n && e - i < kChunkPkts && sum + len[e] + T <= kChunkBytes) {
            const uint64_t nlo = std::min(lo, off[e]), nhi = std::max(hi, off[e] + len[e] + T);
            if (e > i && nhi - nlo > kChunkBytes && nhi - nlo <= 2 * (sum + len[e] + T)) break;
            sum += len[e] + T;
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
        } else {                        // sparse: gather back to back, the FCS places left free
            uint64_t w = 0;
            for (uint64_t q = 0; q < np; q++) {
                std::memcpy(s.h_in + w, arena + off[i + q], len[i + q]);
                s.h_off[q] = w;
                w += len[i + q] + T;
            }
            span = w;
        }
        std::memcpy(s.h_len, len + i, np * 4);
        hipStream_t st = hp->stream;
        if (span) HIPTRY(hipMemcpyAsync(s.d_in, s.h_in, span, hipMemcpyHostToDevice, st), "H2D frames");
        HIPTRY(hipMemcpyAsync(s.d_off, s.h_off, np * 8, hipMemcpyHostToDevice, st), "H2D off");
        HIPTRY(hipMemcpyAsync(s.d_len, s.h_len, np * 4, hipMemcpyHostToDevice, st), "H2D len");
        HIPTRY(hipMemsetAsync(s.d_out + kOutCount, 0, 8, st), "zeroing the count");
        txs::TParams tp{};
        tp.r.base = (uint64_t)s.d_in;
        tp.r.off = s.d_off;
        tp.r.len = s.d_len;
        tp.r.verdict = reinterpret_cast<uint32_t *>(s.d_out);
        tp.r.bad = reinterpret_cast<unsigned long long *>(s.d_out + kOutCount);
        tp.r.n = np;
        tp.r.lo4 = floor4(tp.r.base);
        tp.r.hi4 = ceil4(tp.r.base + kChunkBytes + 64);   // the staging buffer: always more than two lane chunks
        tp.r.bad_mask = count_mask;
        tp.r.zmax = 96;
        tp.fields = reinterpret_cast<txs::Fields *>(s.d_out + kOutFields);
        tp.flags = flags;
        if ((rc = launch(true, tp, hp->dev, cus, st))) return rc;
        HIPTRY(hipMemcpyAsync(s.h_out, s.d_out, np * 4, hipMemcpyDeviceToHost, st), "D2H status");
        HIPTRY(hipMemcpyAsync(s.h_out + kOutCount, s.d_out + kOutCount, 8 + np * 8, hipMemcpyDeviceToHost, st),
               "D2H count and fields");
        HIPTRY(hipEventRecord(s.done, st), "hipEventRecord");
        s.live = true;
        s.i0 = i;
        s.n = np;
        i = e;
        b = (b + 1) % kDepth;
        return 0;
    };
    while (i < n && !rc) rc = step();
    if (rc) {   // never leave a slot that would later be drained into this call's frames
        (void)hipStreamSynchronize(hp->stream);
        for (Slot &s : hp->slot) s.live = false;
    }
    for (Slot &s : hp->slot) {
        const int r2 = drain(s);
        if (!rc) rc = r2;
    }
    hipSetDevice(cur);
    return rc ? (int64_t)rc : (int64_t)count;
}

}  // namespace

extern "C" {

int ether_tx_seal_dev(void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint32_t flags,
                      uint32_t count_mask, uint32_t *status, struct txs_fields *fields, uint64_t *count, uint64_t n,
                      void *stream) {
    int rc = check_flags(flags);
    if (rc) return rc;
    if (n && (!arena || !off || !len)) return fcs::set_error(EINVAL, "null pointer");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (count) HIPTRY(hipMemsetAsync(count, 0, 8, (hipStream_t)stream), "zeroing the count");
    if (n == 0) return 0;
    txs::TParams tp{};
    tp.r.base = (uint64_t)arena;
    tp.r.off = off;
    tp.r.len = len;
    tp.r.verdict = status;
    tp.r.bad = (unsigned long long *)count;
    tp.r.n = n;
    tp.r.lo4 = floor4(tp.r.base);
    tp.r.hi4 = ceil4(tp.r.base + arena_bytes);
    tp.r.bad_mask = count_mask;
    tp.r.zmax = 96;
    tp.fields = reinterpret_cast<txs::Fields *>(fields);
    tp.flags = flags;
    return launch(true, tp, dev, cus, (hipStream_t)stream);
}

int ether_tx_seal_fixed_dev(void *base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags, uint32_t count_mask,
                            uint32_t *status, struct txs_fields *fields, uint64_t *count, void *stream) {
    int rc = check_flags(flags);
    if (rc) return rc;
    if (n && !base) return fcs::set_error(EINVAL, "null pointer");
    const uint64_t T = (flags & TXS_F_FCS) ? 4 : 0;
    if (n > 1 && stride < (uint64_t)len + T)
        return fcs::set_error(EINVAL, "stride %llu < len %u%s", (unsigned long long)stride, len,
                              T ? " + 4 (the FCS place)" : "");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (count) HIPTRY(hipMemsetAsync(count, 0, 8, (hipStream_t)stream), "zeroing the count");
    if (n == 0) return 0;
    txs::TParams tp{};
    tp.r.base = (uint64_t)base;
    tp.r.stride = stride;
    tp.r.flen = len;
    tp.r.verdict = status;
    tp.r.bad = (unsigned long long *)count;
    tp.r.n = n;
    tp.r.lo4 = floor4(tp.r.base);
    tp.r.hi4 = ceil4(tp.r.base + (n - 1) * stride + len + T);
    tp.r.bad_mask = count_mask;
    tp.r.zmax = fcs::mask_bound(len);
    tp.fields = reinterpret_cast<txs::Fields *>(fields);
    tp.flags = flags;
    return launch(false, tp, dev, cus, (hipStream_t)stream);
}

int64_t ether_tx_seal_host(void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint32_t flags,
                           uint32_t count_mask, uint32_t *status, uint64_t n) {
    const int rc = check_flags(flags);
    if (rc) return rc;
    if (n == 0) return 0;
    if (!arena || !off || !len) return fcs::set_error(EINVAL, "null pointer");
    for (uint64_t i = 0; i < n; i++) {
        if (off[i] > arena_bytes || len[i] > arena_bytes - off[i])
            return fcs::set_error(EINVAL, "frame %llu [%llu, +%u) outside the %llu-byte arena", (unsigned long long)i,
                                  (unsigned long long)off[i], len[i], (unsigned long long)arena_bytes);
        if ((flags & TXS_F_FCS) && arena_bytes - off[i] - len[i] < 4)
            return fcs::set_error(EINVAL, "FCS place of frame %llu [%llu, +4) outside the %llu-byte arena",
                                  (unsigned long long)i, (unsigned long long)(off[i] + len[i]),
                                  (unsigned long long)arena_bytes);
    }
    return run_host((uint8_t *)arena, off, len, flags, count_mask, status, n);
}

uint64_t ether_tx_seal_set_dma_threshold(uint64_t frames) { return g_dma_min.exchange(frames); }

// txs::route's decision for a fixed-stride batch, named (no device call).
int fcs_debug_txs_route(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags, char *out, uint64_t cap) {
    const uint64_t T = (flags & TXS_F_FCS) ? 4 : 0;
    txs::TParams tp{};
    tp.r.base = base;
    tp.r.stride = stride;
    tp.r.flen = len;
    tp.r.n = n;
    tp.r.lo4 = floor4(base);
    tp.r.hi4 = n ? ceil4(base + (n - 1) * stride + len + T) : tp.r.lo4;
    tp.flags = flags;
    return copy_name(route_name(txs::route(false, tp, g_dma_min.load(std::memory_order_relaxed))), out, cap);
}

// The kernel the last ether_tx_seal launch of this process actually launched.
int fcs_debug_txs_last_launch(char *out, uint64_t cap) { return copy_name(route_name(txs::last_launch()), out, cap); }

}  // extern "C"
