// host_pipe.hpp — what the host forms of the batch engines (inet, rxv, txs, txf) share: the HIP error
// helpers, the device guard, and a double-buffered H2D -> kernel -> D2H pipeline over chunks of a
// batch. An engine declares its buffers once (BufSpec list), and gives run_pipe two callables:
// issue(slot, stream, i) stages and enqueues the chunk that starts at i, drain(slot) hands a finished
// chunk's results to the caller. Everything else (one pipeline per engine and device, made on first
// use and never freed; the slot cycle; what happens on an error) is here. Not exported.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_chunk.hpp"

namespace hostpipe {

inline int hip_fail(hipError_t e, const char *what) {
    const int err = (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorNoBinaryForGpu ||
                     e == hipErrorInvalidDeviceFunction || e == hipErrorInvalidImage)
                        ? ENODEV
                        : (e == hipErrorOutOfMemory ? ENOMEM : EIO);
    return fcs::set_error(err, "%s: %s", what, hipGetErrorString(e));
}

#define HIPTRY(expr, what)                                           \
    do {                                                             \
        hipError_t e_ = (expr);                                      \
        if (e_ != hipSuccess) return hostpipe::hip_fail(e_, what);   \
    } while (0)

inline uint64_t floor4(uint64_t x) { return x & ~3ull; }
inline uint64_t ceil4(uint64_t x) { return (x + 3) & ~3ull; }

inline int copy_name(const char *r, char *out, uint64_t cap) {
    if (!out || cap == 0) return -EINVAL;
    const uint64_t k = std::min<uint64_t>(std::strlen(r), cap - 1);
    std::memcpy(out, r, k);
    out[k] = 0;
    return (int)k;
}

// Makes `dev` current for the scope and restores the caller's device on exit (a host-batch call
// must not leave a multi-GPU caller's thread on another device: its next *_dev call resolves the
// device from the thread's current one).
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        err = hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) hipSetDevice(prev);
    }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};

struct BufSpec {
    uint64_t bytes;
    const char *what;   // names the buffer in an allocation error
};

// One chunk in flight: buf[k] is the engine's k-th BufSpec as a device array and its pinned twin.
struct Slot {
    struct Buf {
        void *d = nullptr, *h = nullptr;
    };
    std::vector<Buf> buf;
    hipEvent_t done = nullptr;
    bool live = false;        // set by issue once the chunk's work is enqueued; cleared when drained
    uint64_t i0 = 0, n = 0;   // the chunk's place in the caller's arrays, for drain
    template <class T> T *d(int k) const { return static_cast<T *>(buf[k].d); }
    template <class T> T *h(int k) const { return static_cast<T *>(buf[k].h); }
};

struct HostPipe {
    std::mutex mu;
    hipStream_t stream = nullptr;
    std::vector<Slot> slot;
};

inline void free_pipe(HostPipe &hp) {
    for (Slot &s : hp.slot) {
        if (s.done) (void)hipEventDestroy(s.done);
        for (Slot::Buf &b : s.buf) {
            if (b.d) (void)hipFree(b.d);
            if (b.h) (void)hipHostFree(b.h);
        }
    }
    hp.slot.clear();
    if (hp.stream) (void)hipStreamDestroy(hp.stream);
    hp.stream = nullptr;
}

inline int alloc_pipe(HostPipe &hp, int dev, int depth, const std::vector<BufSpec> &bufs) {
    DeviceGuard dg(dev);
    HIPTRY(dg.err, "hipSetDevice");
    HIPTRY(hipStreamCreateWithFlags(&hp.stream, hipStreamNonBlocking), "hipStreamCreate");
    hp.slot.resize(depth);
    for (Slot &s : hp.slot) {
        s.buf.resize(bufs.size());
        Slot::Buf *b = s.buf.data();
        for (const BufSpec &spec : bufs) {
            const std::string what = std::string("(") + spec.what + ")";
            HIPTRY(hipMalloc(&b->d, spec.bytes), ("hipMalloc" + what).c_str());
            HIPTRY(hipHostMalloc(&b->h, spec.bytes, hipHostMallocDefault), ("hipHostMalloc" + what).c_str());
            b++;
        }
        HIPTRY(hipEventCreateWithFlags(&s.done, hipEventDisableTiming), "hipEventCreate");
    }
    return 0;
}

// The pipeline of engine `Engine` (a tag type of the engine's own: every engine has its own registry,
// so that no two share staging or wait for one another) on device `dev`.
template <class Engine>
int get_pipe(int dev, int depth, const std::vector<BufSpec> &bufs, HostPipe **out) {
    static std::mutex g_pipes_mu;
    static std::map<int, std::unique_ptr<HostPipe>> g_pipes;
    std::lock_guard<std::mutex> lk(g_pipes_mu);
    auto &up = g_pipes[dev];
    if (!up) {
        auto hp = std::make_unique<HostPipe>();
        const int rc = alloc_pipe(*hp, dev, depth, bufs);
        if (rc) {   // a half-built pipeline holds nothing: the next call starts over
            free_pipe(*hp);
            return rc;
        }
        up = std::move(hp);
    }
    *out = up.get();
    return 0;
}

// Runs frames [0, n) through the pipeline: int64_t issue(Slot &, hipStream_t, uint64_t i) returns the
// next i (having set the slot's i0, n and live unless the chunk needed no device work) or -errno;
// void drain(Slot &) is called once the slot's event has passed. The caller's device is current
// again on return, whatever the return.
template <class Engine, class Issue, class Drain>
int run_pipe(int dev, int depth, const std::vector<BufSpec> &bufs, uint64_t n, Issue &&issue, Drain &&drain) {
    HostPipe *hp = nullptr;
    int rc = get_pipe<Engine>(dev, depth, bufs, &hp);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(hp->mu);
    DeviceGuard dg(dev);
    HIPTRY(dg.err, "hipSetDevice");
    auto retire = [&](Slot &s) -> int {
        if (!s.live) return 0;
        HIPTRY(hipEventSynchronize(s.done), "hipEventSynchronize");
        drain(s);
        s.live = false;
        return 0;
    };
    auto step = [&](Slot &s, uint64_t &i) -> int {
        const int rc = retire(s);
        if (rc) return rc;
        const int64_t next = issue(s, hp->stream, i);
        if (next < 0) return (int)next;
        if (s.live) HIPTRY(hipEventRecord(s.done, hp->stream), "hipEventRecord");
        i = (uint64_t)next;
        return 0;
    };
    uint64_t i = 0;
    for (int b = 0; i < n && !rc; b = (b + 1) % depth) rc = step(hp->slot[b], i);
    if (rc) {   // never leave a slot that would later be drained into this call's results
        (void)hipStreamSynchronize(hp->stream);
        for (Slot &s : hp->slot) s.live = false;
    }
    for (Slot &s : hp->slot) {
        const int r2 = retire(s);
        if (!rc) rc = r2;
    }
    return rc;
}

// For the engines that chunk with host_chunk.hpp and keep frames, offsets and lengths in their
// buffers 0, 1 and 2: stages chunk [i, c.e) of (arena, off, len) and enqueues its three H2D copies.
inline int stage_h2d(Slot &s, hipStream_t st, const uint8_t *arena, const uint64_t *off, const uint32_t *len, uint64_t i,
                     const hostchunk::Cut &c, uint64_t K, uint64_t T, const char *what) {
    const uint64_t np = c.e - i;
    const uint64_t span = hostchunk::stage(arena, off, len, i, c, K, T, s.h<uint8_t>(0), s.h<uint64_t>(1), fcs::staging_copy);
    std::memcpy(s.h<uint32_t>(2), len + i, np * 4);
    if (span) HIPTRY(hipMemcpyAsync(s.d<void>(0), s.h<void>(0), span, hipMemcpyHostToDevice, st), what);
    HIPTRY(hipMemcpyAsync(s.d<void>(1), s.h<void>(1), np * 8, hipMemcpyHostToDevice, st), "H2D off");
    HIPTRY(hipMemcpyAsync(s.d<void>(2), s.h<void>(2), np * 4, hipMemcpyHostToDevice, st), "H2D len");
    return 0;
}

// A device plan's scratch, which lives on the stream between its launches: hipError_t fn(void *mem)
// fills it and launches; it is freed on the stream whatever fn returns, and fn's error is the one
// reported first.
template <class Fn>
int with_stream_scratch(uint64_t bytes, hipStream_t st, Fn &&fn) {
    void *mem = nullptr;
    HIPTRY(hipMallocAsync(&mem, bytes, st), "hipMallocAsync(plan scratch)");
    const hipError_t e = fn(mem), e2 = hipFreeAsync(mem, st);
    HIPTRY(e, "launching the plan kernels");
    HIPTRY(e2, "hipFreeAsync(plan scratch)");
    return 0;
}

// The items of each chunk of this thread's last host call of an engine (tests read it back through
// the engine's fcs_debug_*_last_host_chunks).
struct ChunkLog {
    std::vector<uint64_t> items;
    void clear() { items.clear(); }
    void add(uint64_t n) { items.push_back(n); }
    int64_t report(uint64_t *out, uint64_t cap) const {
        for (uint64_t k = 0; out && k < cap && k < items.size(); k++) out[k] = items[k];
        return (int64_t)items.size();
    }
};

}  // namespace hostpipe
