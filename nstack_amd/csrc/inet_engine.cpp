// inet_engine.cpp — the C ABI of include/nstack_inet.h around inet_kernel.hip.
//
// Device forms validate and launch; the host form runs the double-buffered H2D -> kernel -> D2H
// pipeline of host_pipe.hpp in 128 MiB chunks on the engine's first GPU, cut and staged by
// host_chunk.hpp (packets of a chunk are copied as one span when they lie densely, gathered into
// the pinned staging buffer otherwise). The single-packet forms keep the reference functions'
// signatures (src/ip.c:39, src/tcp.c:167, src/udp.c:136) and, like them, have no error channel: on
// an engine failure they abort with the reason.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../include/nstack_fcs.h"
#include "../../include/nstack_inet.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_pipe.hpp"
#include "inet_launch.hpp"

using namespace hostpipe;

namespace {

std::atomic<uint64_t> g_flat_min{16384};   // see inet_csum_set_flat_threshold
std::atomic<uint64_t> g_dma_min{16384};    // see inet_csum_set_dma_threshold

// launch_inet with the work counter the LDS-DMA route takes (the same route_inet decision the
// launcher makes), leased from the FCS engine's ring of device `dev` for this launch.
int launch_counted(bool var, int mode, inet::IParams &p, int dev, int cus, hipStream_t st) {
    const uint64_t flat_min = g_flat_min.load(std::memory_order_relaxed), dma_min = g_dma_min.load(std::memory_order_relaxed);
    auto go = [&](unsigned long long *ctr) -> int {
        p.ctr = ctr;
        HIPTRY(inet::launch_inet(var, mode, p, cus, flat_min, dma_min, st), "launching the inet kernel");
        return 0;
    };
    if (inet::route_inet(var, p, flat_min, dma_min) == inet::Route::kDma)
        return fcs::launch_with_counter(dev, (void *)st, go);
    return go(nullptr);
}

int check_mode(int mode, const uint32_t *addr) {
    if (mode != INET_CSUM_IP && mode != INET_CSUM_TCP && mode != INET_CSUM_UDP)
        return fcs::set_error(EINVAL, "unknown checksum mode %d", mode);
    if (mode != INET_CSUM_IP && !addr) return fcs::set_error(EINVAL, "mode %d needs the address array", mode);
    return 0;
}

// ---- host pipeline ----
constexpr uint64_t kChunkBytes = 128ull << 20;
constexpr uint64_t kChunkPkts = 1ull << 20;
constexpr int kDepth = 2;

struct InetPipe;   // names this engine's pipelines (host_pipe.hpp)
enum { kIn, kOff, kLen, kAddr, kOut };
const std::vector<BufSpec> kBufs = {{kChunkBytes + 64, "inet staging"}, {kChunkPkts * 8, "off"},
                                    {kChunkPkts * 4, "len"},            {kChunkPkts * 8, "addr"},
                                    {kChunkPkts * 2, "out"}};

int run_host(int mode, const uint8_t *arena, const uint64_t *off, const uint32_t *len, const uint32_t *addr,
             uint16_t *out, uint64_t n) {
    int dev = 0, cus = 0;
    const int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    auto issue = [&](Slot &s, hipStream_t st, uint64_t i) -> int64_t {
        const hostchunk::Cut c = hostchunk::cut(off, len, i, n, kChunkBytes, kChunkPkts, 0);
        if (c.e == i)
            return fcs::set_error(EINVAL, "packet %llu of %u bytes exceeds the %llu-byte host chunk",
                                  (unsigned long long)i, len[i], (unsigned long long)kChunkBytes);
        const uint64_t np = c.e - i;
        int rc = stage_h2d(s, st, arena, off, len, i, c, kChunkBytes, 0, "H2D packets");
        if (rc) return rc;
        if (addr) {
            std::memcpy(s.h<uint32_t>(kAddr), addr + 2 * i, np * 8);
            HIPTRY(hipMemcpyAsync(s.d<void>(kAddr), s.h<void>(kAddr), np * 8, hipMemcpyHostToDevice, st), "H2D addr");
        }
        inet::IParams p{};
        p.base = (uint64_t)s.d<void>(kIn);
        p.off = s.d<uint64_t>(kOff);
        p.len = s.d<uint32_t>(kLen);
        p.addr = addr ? s.d<uint32_t>(kAddr) : nullptr;
        p.out = s.d<uint16_t>(kOut);
        p.n = np;
        if ((rc = launch_counted(true, mode, p, dev, cus, st))) return rc;
        HIPTRY(hipMemcpyAsync(s.h<void>(kOut), s.d<void>(kOut), np * 2, hipMemcpyDeviceToHost, st), "D2H checksums");
        s.i0 = i;
        s.n = np;
        s.live = true;
        return (int64_t)c.e;
    };
    auto drain = [&](Slot &s) { std::memcpy(out + s.i0, s.h<uint16_t>(kOut), s.n * 2); };
    return run_pipe<InetPipe>(dev, kDepth, kBufs, n, issue, drain);
}

uint16_t single_or_die(int mode, const void *dp, size_t bsize, uint32_t src, uint32_t dst, const char *name) {
    if (bsize > UINT32_MAX) {
        std::fprintf(stderr, "nstack_fcs: %s: %zu-byte packet exceeds the engine's 32-bit length\n", name, bsize);
        std::abort();
    }
    const uint64_t off = 0;
    const uint32_t len = (uint32_t)bsize, addr[2] = {src, dst};
    uint16_t out = 0;
    static const uint8_t kEmpty[1] = {0};
    const int rc = run_host(mode, bsize ? (const uint8_t *)dp : kEmpty, &off, &len, addr, &out, 1);
    if (rc) {
        std::fprintf(stderr, "nstack_fcs: %s: no usable GPU engine: %s\n", name, fcs_last_error());
        std::abort();
    }
    return out;
}

}  // namespace

extern "C" {

int inet_csum_batch_dev(int mode, const void *arena, uint64_t arena_bytes, const uint64_t *off,
                        const uint32_t *len, const uint32_t *addr, uint16_t *out, uint64_t n, void *stream) {
    int rc = check_mode(mode, addr);
    if (rc || n == 0) return rc;
    if (!arena || !off || !len || !out) return fcs::set_error(EINVAL, "null pointer");
    (void)arena_bytes;   // device arrays: bounds are the caller's contract (as ether_fcs_batch_dev)
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    inet::IParams p{};
    p.base = (uint64_t)arena;
    p.off = off;
    p.len = len;
    p.addr = addr;
    p.out = out;
    p.n = n;
    return launch_counted(true, mode, p, dev, cus, (hipStream_t)stream);
}

int inet_csum_fixed_dev(int mode, const void *base, uint64_t stride, uint32_t len, uint64_t n,
                        const uint32_t *addr, uint16_t *out, void *stream) {
    int rc = check_mode(mode, addr);
    if (rc || n == 0) return rc;
    if (!base || !out) return fcs::set_error(EINVAL, "null pointer");
    if (n > 1 && stride < len) return fcs::set_error(EINVAL, "stride %llu < len %u", (unsigned long long)stride, len);
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    inet::IParams p{};
    p.base = (uint64_t)base;
    p.stride = stride;
    p.flen = len;
    p.addr = addr;
    p.out = out;
    p.n = n;
    return launch_counted(false, mode, p, dev, cus, (hipStream_t)stream);
}

int inet_csum_batch_host(int mode, const void *arena, uint64_t arena_bytes, const uint64_t *off,
                         const uint32_t *len, const uint32_t *addr, uint16_t *out, uint64_t n) {
    int rc = check_mode(mode, addr);
    if (rc || n == 0) return rc;
    if (!arena || !off || !len || !out) return fcs::set_error(EINVAL, "null pointer");
    for (uint64_t i = 0; i < n; i++)
        if (off[i] > arena_bytes || len[i] > arena_bytes - off[i])
            return fcs::set_error(EINVAL, "packet %llu [%llu, +%u) outside the %llu-byte arena",
                                  (unsigned long long)i, (unsigned long long)off[i], len[i],
                                  (unsigned long long)arena_bytes);
    return run_host(mode, (const uint8_t *)arena, off, len, addr, out, n);
}

uint64_t inet_csum_set_flat_threshold(uint64_t packets) { return g_flat_min.exchange(packets); }

uint64_t inet_csum_set_dma_threshold(uint64_t packets) { return g_dma_min.exchange(packets); }

uint16_t inet_ip_checksum(const void *dp, size_t bsize) {
    return single_or_die(INET_CSUM_IP, dp, bsize, 0, 0, "inet_ip_checksum");
}

uint16_t inet_tcp_checksum(uint32_t src, uint32_t dst, const void *dp, size_t bsize) {
    return single_or_die(INET_CSUM_TCP, dp, bsize, src, dst, "inet_tcp_checksum");
}

uint16_t inet_udp_checksum(const void *dp, size_t len, uint32_t src, uint32_t dst) {
    return single_or_die(INET_CSUM_UDP, dp, len, src, dst, "inet_udp_checksum");
}

}  // extern "C"
