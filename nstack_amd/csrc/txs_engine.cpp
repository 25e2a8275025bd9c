// txs_engine.cpp — the C ABI of include/nstack_txs.h around txs_kernel.hip.
//
// Device forms validate and launch; the host form runs the double-buffered H2D -> kernel -> D2H
// pipeline of host_pipe.hpp in 64 MiB chunks on the engine's first GPU, in staging of its own, cut
// and staged by host_chunk.hpp with every frame's FCS place counted to it. Only the status word and
// the 8-byte fields record of each frame travel back: the caller's frames are patched from them on
// the host (where to write follows from the status bits and the header), the frame bytes do not
// travel back. No CPU path: a failure is returned, never answered on the host, and the FCS engine's
// host-batch and fallback counters are not touched.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cerrno>
#include <cstring>

#include "../../include/nstack_txs.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_pipe.hpp"
#include "txs_launch.hpp"

static_assert(sizeof(txs_fields) == 8 && sizeof(txs::Fields) == 8, "the fields record is 8 bytes");

using namespace hostpipe;

namespace {

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

uint64_t fcs_place(uint32_t flags) { return (flags & TXS_F_FCS) ? 4 : 0; }   // bytes behind each frame that belong to it

// The parameters of a variable batch whose frames lie in the `bytes` bytes at `base`.
txs::TParams var_params(uint64_t base, uint64_t bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                        uint32_t flags, uint32_t count_mask, uint32_t *status, void *fields, void *count) {
    txs::TParams tp{};
    tp.r.base = base;
    tp.r.off = off;
    tp.r.len = len;
    tp.r.verdict = status;
    tp.r.bad = (unsigned long long *)count;
    tp.r.n = n;
    tp.r.lo4 = floor4(base);
    tp.r.hi4 = ceil4(base + bytes);
    tp.r.bad_mask = count_mask;
    tp.r.zmax = 96;
    tp.fields = (txs::Fields *)fields;
    tp.flags = flags;
    return tp;
}

// The parameters of a fixed-stride batch: what the launch gets and what fcs_debug_txs_route names.
txs::TParams fixed_params(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags,
                          uint32_t count_mask, uint32_t *status, void *fields, void *count) {
    txs::TParams tp{};
    tp.r.base = base;
    tp.r.stride = stride;
    tp.r.flen = len;
    tp.r.verdict = status;
    tp.r.bad = (unsigned long long *)count;
    tp.r.n = n;
    tp.r.lo4 = floor4(base);
    tp.r.hi4 = n ? ceil4(base + (n - 1) * stride + len + fcs_place(flags)) : tp.r.lo4;
    tp.r.bad_mask = count_mask;
    tp.r.zmax = fcs::mask_bound(len);
    tp.fields = (txs::Fields *)fields;
    tp.flags = flags;
    return tp;
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

struct TxsPipe;   // names this engine's pipelines (host_pipe.hpp)
enum { kIn, kOff, kLen, kOut };
const std::vector<BufSpec> kBufs = {{kChunkBytes + 64, "txs staging"}, {kChunkPkts * 8, "off"},
                                    {kChunkPkts * 4, "len"},           {kOutBytes, "status"}};

int64_t run_host(uint8_t *arena, const uint64_t *off, const uint32_t *len, uint32_t flags, uint32_t count_mask,
                 uint32_t *status, uint64_t n) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    const uint64_t T = fcs_place(flags);
    uint64_t count = 0;
    auto issue = [&](Slot &s, hipStream_t st, uint64_t i) -> int64_t {
        const hostchunk::Cut c = hostchunk::cut(off, len, i, n, kChunkBytes, kChunkPkts, T);
        if (c.e == i)
            return fcs::set_error(EINVAL, "frame %llu of %u bytes exceeds the %llu-byte host chunk",
                                  (unsigned long long)i, len[i], (unsigned long long)kChunkBytes);
        const uint64_t np = c.e - i;
        int rc = stage_h2d(s, st, arena, off, len, i, c, kChunkBytes, T, "H2D frames");
        if (rc) return rc;
        uint8_t *d_out = s.d<uint8_t>(kOut), *h_out = s.h<uint8_t>(kOut);
        HIPTRY(hipMemsetAsync(d_out + kOutCount, 0, 8, st), "zeroing the count");
        // the arena is the staging buffer: always more than two lane chunks
        txs::TParams tp = var_params((uint64_t)s.d<void>(kIn), kChunkBytes + 64, s.d<uint64_t>(kOff), s.d<uint32_t>(kLen),
                                     np, flags, count_mask, (uint32_t *)d_out, d_out + kOutFields, d_out + kOutCount);
        if ((rc = launch(true, tp, dev, cus, st))) return rc;
        HIPTRY(hipMemcpyAsync(h_out, d_out, np * 4, hipMemcpyDeviceToHost, st), "D2H status");
        HIPTRY(hipMemcpyAsync(h_out + kOutCount, d_out + kOutCount, 8 + np * 8, hipMemcpyDeviceToHost, st),
               "D2H count and fields");
        s.i0 = i;
        s.n = np;
        s.live = true;
        return (int64_t)c.e;
    };
    auto drain = [&](Slot &s) {
        const uint8_t *h_out = s.h<uint8_t>(kOut);
        const uint32_t *st = reinterpret_cast<const uint32_t *>(h_out);
        const txs::Fields *fl = reinterpret_cast<const txs::Fields *>(h_out + kOutFields);
        for (uint64_t q = 0; q < s.n; q++) patch_host(arena + off[s.i0 + q], len[s.i0 + q], flags, st[q], fl[q]);
        if (status) std::memcpy(status + s.i0, st, s.n * 4);
        uint64_t b = 0;
        std::memcpy(&b, h_out + kOutCount, 8);
        count += b;
    };
    rc = run_pipe<TxsPipe>(dev, kDepth, kBufs, n, issue, drain);
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
    txs::TParams tp = var_params((uint64_t)arena, arena_bytes, off, len, n, flags, count_mask, status, fields, count);
    return launch(true, tp, dev, cus, (hipStream_t)stream);
}

int ether_tx_seal_fixed_dev(void *base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags, uint32_t count_mask,
                            uint32_t *status, struct txs_fields *fields, uint64_t *count, void *stream) {
    int rc = check_flags(flags);
    if (rc) return rc;
    if (n && !base) return fcs::set_error(EINVAL, "null pointer");
    const uint64_t T = fcs_place(flags);
    if (n > 1 && stride < (uint64_t)len + T)
        return fcs::set_error(EINVAL, "stride %llu < len %u%s", (unsigned long long)stride, len,
                              T ? " + 4 (the FCS place)" : "");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (count) HIPTRY(hipMemsetAsync(count, 0, 8, (hipStream_t)stream), "zeroing the count");
    if (n == 0) return 0;
    txs::TParams tp = fixed_params((uint64_t)base, stride, len, n, flags, count_mask, status, fields, count);
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
    const txs::TParams tp = fixed_params(base, stride, len, n, flags, 0, nullptr, nullptr, nullptr);
    return copy_name(route_name(txs::route(false, tp, g_dma_min.load(std::memory_order_relaxed))), out, cap);
}

// The kernel the last ether_tx_seal launch of this process actually launched.
int fcs_debug_txs_last_launch(char *out, uint64_t cap) { return copy_name(route_name(txs::last_launch()), out, cap); }

}  // extern "C"
