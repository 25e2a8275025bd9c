// txf_engine.cpp — the C ABI of include/nstack_txf.h and include/nstack_txd.h around txf_kernel.hip.
//
// Device forms validate and launch. The host form plans on the host (txf_plan.hpp), checks every
// datagram and the slot capacity, and then runs the double-buffered H2D -> kernel -> D2H pipeline of
// host_pipe.hpp over datagram ranges on the engine's first GPU, in staging and with a cut of its own:
// a chunk's datagrams are gathered back to back, its frames come back slot by slot and only their
// F (+ 4) bytes are copied into the caller's arena. No CPU path: a failure is returned, never
// answered on the host, and the FCS engine's host-batch and fallback counters are not touched.
// ip_tx_frame_l4_* (nstack_txd.h) are the same two forms with the kernel's L4 variant: the checks,
// the leases, the plan, the cut and the constants are shared. ip_tx_tso_* (nstack_tso.h) are the same
// again with the segmenting variant, the plan of tso_plan.hpp and an mss array staged per chunk.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstring>
#include <vector>

#include "../../include/nstack_tso.h"
#include "../../include/nstack_txd.h"
#include "../../include/nstack_txf.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_pipe.hpp"
#include "txf_launch.hpp"

static_assert(sizeof(txf_l2) == 12, "the MAC record is 12 bytes");

using namespace hostpipe;
using txf::Mode;

namespace {

int check_call(uint32_t mtu, uint32_t flags, uint32_t known = txf::kKnownFlags) {
    if (flags & ~known) return fcs::set_error(EINVAL, "unknown flag bits 0x%x", flags & ~known);
    if (mtu < txf::kMinMtu || mtu > txf::kMaxMtu)
        return fcs::set_error(EINVAL, "mtu %u outside [%u, %u]", mtu, txf::kMinMtu, txf::kMaxMtu);
    return 0;
}

int check_slot(uint32_t mtu, uint32_t flags, uint64_t slot, uint64_t slots) {
    if (slot < txf::min_slot(mtu, flags))
        return fcs::set_error(EINVAL, "slot %llu < %llu (14 + mtu, at least 70%s)", (unsigned long long)slot,
                              (unsigned long long)txf::min_slot(mtu, flags),
                              (flags & txf::kFlagFcs) ? ", + 4 for the FCS" : "");
    if (slots && slot > UINT64_MAX / slots) return fcs::set_error(EINVAL, "slot * slots overflows");
    return 0;
}

// launch_txf with the work counter its rows take their datagrams from, leased from the FCS engine's
// ring of device `dev` for this launch.
int launch(txf::FParams &p, Mode mode, int dev, int cus, hipStream_t st) {
    return fcs::launch_with_counter(dev, (void *)st, [&](unsigned long long *ctr) -> int {
        p.ctr = ctr;
        HIPTRY(txf::launch_txf(p, mode, cus, st), mode == Mode::kTso  ? "launching the tso kernel"
                                                  : mode == Mode::kL4 ? "launching the txd kernel"
                                                                      : "launching the txf kernel");
        return 0;
    });
}

// ---- host pipeline ----
constexpr uint64_t kInBytes = 32ull << 20;     // a chunk's datagrams
constexpr uint64_t kOutBytes = 64ull << 20;    // a chunk's slots
constexpr uint64_t kChunkDgs = 1ull << 18;
// Sizes the flen staging only; as a bound on a chunk it cannot bind: at the smallest slot (70 bytes)
// 2^20 frames are 70 MiB, more than kOutBytes, so the slot bound always cuts first.
constexpr uint64_t kChunkFrames = 1ull << 20;
constexpr int kDepth = 2;

struct TxfPipe;   // names this engine's pipelines (host_pipe.hpp)
enum { kIn, kOff, kLen, kL2, kOut, kFlen };   // kOff: off[kChunkDgs], then first[kChunkDgs]; kLen: len, then the u16 mss
const std::vector<BufSpec> kBufs = {{kInBytes + 64, "txf staging"}, {kChunkDgs * 16, "off"},   {kChunkDgs * 6, "len, mss"},
                                    {kChunkDgs * 12, "l2"},         {kOutBytes, "txf frames"}, {kChunkFrames * 4, "flen"}};

// first[0..n] is the host plan; frames of datagrams [i, e) go to slots [first[i], first[e]).
int64_t run_host(Mode mode, const uint8_t *dgram, const uint64_t *off, const uint32_t *len, const uint8_t *l2,
                 const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags, const uint64_t *first, uint8_t *out,
                 uint64_t slot, uint32_t *flen) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    const uint64_t T = (flags & txf::kFlagFcs) ? 4 : 0;
    // a refused datagram travels as an empty one: its status is the host plan's
    auto glen = [&](uint64_t q) -> uint32_t { return first[q + 1] > first[q] ? len[q] : 0u; };
    auto issue = [&](Slot &s, hipStream_t st, uint64_t i) -> int64_t {
        const uint32_t *blob = nullptr;
        int rc = (flags & txf::kFlagFcs) ? fcs::device_tables(dev, &blob) : 0;
        if (rc) return rc;
        uint64_t e = i, sum = 0;
        while (e < n && e - i < kChunkDgs && sum + glen(e) <= kInBytes && first[e + 1] - first[i] <= kChunkFrames &&
               (first[e + 1] - first[i]) * slot <= kOutBytes) {
            sum += glen(e);
            e++;
        }
        if (e == i)   // checked before any work (ether_tx_frame_host): cannot happen
            return fcs::set_error(EINVAL, "datagram %llu exceeds the host chunk", (unsigned long long)i);
        const uint64_t np = e - i, frames = first[e] - first[i];
        if (!frames) return (int64_t)e;   // a chunk of refused datagrams needs no device
        uint8_t *h_in = s.h<uint8_t>(kIn);
        uint64_t *h_off = s.h<uint64_t>(kOff), *d_off = s.d<uint64_t>(kOff), w = 0;
        for (uint64_t q = 0; q < np; q++) {
            const uint32_t gl = glen(i + q);
            std::memcpy(h_in + w, dgram + off[i + q], gl);
            h_off[q] = w;
            h_off[kChunkDgs + q] = first[i + q] - first[i];
            s.h<uint32_t>(kLen)[q] = gl;
            w += gl;
        }
        const uint64_t nl2 = (flags & txf::kFlagL2One) ? 1 : np;
        std::memcpy(s.h<void>(kL2), l2 + ((flags & txf::kFlagL2One) ? 0 : i * 12), nl2 * 12);
        if (w) HIPTRY(hipMemcpyAsync(s.d<void>(kIn), h_in, w, hipMemcpyHostToDevice, st), "H2D datagrams");
        HIPTRY(hipMemcpyAsync(d_off, h_off, np * 8, hipMemcpyHostToDevice, st), "H2D off");
        HIPTRY(hipMemcpyAsync(d_off + kChunkDgs, h_off + kChunkDgs, np * 8, hipMemcpyHostToDevice, st), "H2D first");
        HIPTRY(hipMemcpyAsync(s.d<void>(kLen), s.h<void>(kLen), np * 4, hipMemcpyHostToDevice, st), "H2D len");
        HIPTRY(hipMemcpyAsync(s.d<void>(kL2), s.h<void>(kL2), nl2 * 12, hipMemcpyHostToDevice, st), "H2D l2");
        const uint16_t *d_mss = nullptr;   // nstack_tso.h: the chunk's mss entries behind its len[]
        if (mss) {
            const uint64_t nm = (flags & txf::kFlagMssOne) ? 1 : np;
            uint16_t *h_mss = reinterpret_cast<uint16_t *>(s.h<uint32_t>(kLen) + kChunkDgs);
            std::memcpy(h_mss, mss + ((flags & txf::kFlagMssOne) ? 0 : i), nm * 2);
            d_mss = reinterpret_cast<const uint16_t *>(s.d<uint32_t>(kLen) + kChunkDgs);
            HIPTRY(hipMemcpyAsync((void *)d_mss, h_mss, nm * 2, hipMemcpyHostToDevice, st), "H2D mss");
        }
        txf::FParams p{};
        p.dg = (uint64_t)s.d<void>(kIn);
        p.lo4 = floor4(p.dg);
        p.hi4 = ceil4(p.dg + kInBytes + 64);   // the staging buffer
        p.off = d_off;
        p.len = s.d<uint32_t>(kLen);
        p.n = np;
        p.mtu = mtu;
        p.flags = flags;
        p.l2 = s.d<uint8_t>(kL2);
        p.first = d_off + kChunkDgs;
        p.out = (uint64_t)s.d<void>(kOut);
        p.slot = slot;
        p.slots = frames;
        p.flen = s.d<uint32_t>(kFlen);
        p.blob = blob;
        p.mss = d_mss;
        if ((rc = launch(p, mode, dev, cus, st))) return rc;
        HIPTRY(hipMemcpyAsync(s.h<void>(kOut), s.d<void>(kOut), frames * slot, hipMemcpyDeviceToHost, st), "D2H frames");
        HIPTRY(hipMemcpyAsync(s.h<void>(kFlen), s.d<void>(kFlen), frames * 4, hipMemcpyDeviceToHost, st), "D2H flen");
        s.i0 = first[i];   // the chunk's first slot and its frames
        s.n = frames;
        s.live = true;
        return (int64_t)e;
    };
    auto drain = [&](Slot &s) {
        for (uint64_t q = 0; q < s.n; q++) {
            const uint32_t F = s.h<uint32_t>(kFlen)[q];
            std::memcpy(out + (s.i0 + q) * slot, s.h<uint8_t>(kOut) + q * slot, F + T);
            if (flen) flen[s.i0 + q] = F;
        }
    };
    rc = run_pipe<TxfPipe>(dev, kDepth, kBufs, n, issue, drain);
    return rc ? (int64_t)rc : (int64_t)first[n];
}

const char *route_name(txf::Route r) {
    switch (r) {
    case txf::Route::kGeneralFcs: return "general-fcs";
    case txf::Route::kGeneral: return "general";
    case txf::Route::kGeneralL4Fcs: return "general-l4-fcs";
    case txf::Route::kGeneralL4: return "general-l4";
    case txf::Route::kTsoFcs: return "tso-fcs";
    case txf::Route::kTso: return "tso";
    default: return "none";
    }
}

uint32_t known_flags(Mode mode) {
    return mode == Mode::kTso ? txf::kKnownFlagsTso : (mode == Mode::kL4 ? txf::kKnownFlagsL4 : txf::kKnownFlags);
}

// The device build of the three headers (Mode::kL4: ip_tx_frame_l4_dev; Mode::kTso: ip_tx_tso_dev, mss
// device memory or null).
int frame_dev(Mode mode, const uint16_t *mss, const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
              const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, const uint64_t *first, void *out,
              uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status, uint32_t *fcs_out, void *stream) {
    int rc = check_call(mtu, flags, known_flags(mode));
    if (rc || (rc = check_slot(mtu, flags, slot, slots))) return rc;
    if (n && (!dgram || !off || !len || !l2 || !first || (!out && slots))) return fcs::set_error(EINVAL, "null pointer");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (n == 0) return 0;
    txf::FParams p{};
    p.dg = (uint64_t)dgram;
    p.lo4 = floor4(p.dg);
    p.hi4 = ceil4(p.dg + dgram_bytes);
    p.off = off;
    p.len = len;
    p.n = n;
    p.mtu = mtu;
    p.flags = flags;
    p.l2 = reinterpret_cast<const uint8_t *>(l2);
    p.first = first;
    p.out = (uint64_t)out;
    p.slot = slot;
    p.slots = slots;
    p.flen = flen;
    p.status = status;
    p.fcs = fcs_out;
    p.mss = mss;
    if ((flags & txf::kFlagFcs) && (rc = fcs::device_tables(dev, &p.blob))) return rc;
    return launch(p, mode, dev, cus, (hipStream_t)stream);
}

// The host form of the three headers (Mode::kL4: ip_tx_frame_l4_host, whose status words get the L4
// bits; Mode::kTso: ip_tx_tso_host, planned by tso_plan.hpp, mss host memory or null).
int64_t frame_host(Mode mode, const uint16_t *mss, const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                   const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, void *out, uint64_t slot,
                   uint64_t slots, uint32_t *flen, uint32_t *status) {
    int rc = check_call(mtu, flags, known_flags(mode));
    if (rc || (rc = check_slot(mtu, flags, slot, slots))) return rc;
    if (n == 0) return 0;
    if (!dgram || !off || !len || !l2 || (!out && slots)) return fcs::set_error(EINVAL, "null pointer");
    std::vector<uint64_t> first(n + 1);
    std::vector<uint32_t> st(n);
    uint64_t bad = 0;
    const int prc = mode == Mode::kTso ? txf::tso_plan_batch((const uint8_t *)dgram, dgram_bytes, off, len, mss, n, mtu, flags,
                                                             st.data(), first.data(), &bad)
                                       : txf::plan_batch((const uint8_t *)dgram, dgram_bytes, off, len, n, mtu, flags,
                                                         st.data(), first.data(), &bad);
    if (prc)
        return fcs::set_error(EINVAL, "datagram %llu [%llu, +%u) outside the %llu-byte arena", (unsigned long long)bad,
                              (unsigned long long)off[bad], len[bad], (unsigned long long)dgram_bytes);
    if (first[n] > slots)
        return fcs::set_error(ENOSPC, "%llu frames need more than the %llu slots given", (unsigned long long)first[n],
                              (unsigned long long)slots);
    for (uint64_t i = 0; i < n; i++)
        if ((first[i + 1] - first[i]) * slot > kOutBytes)
            return fcs::set_error(EINVAL, "datagram %llu: %llu slots of %llu bytes exceed the %llu-byte host chunk",
                                  (unsigned long long)i, (unsigned long long)(first[i + 1] - first[i]),
                                  (unsigned long long)slot, (unsigned long long)kOutBytes);
    if (mode == Mode::kL4 && status) {   // nstack_txd.h rule 4, as the kernel states it
        for (uint64_t i = 0; i < n; i++) {
            if (st[i] & (txf::kBadHdr | txf::kBadLen)) continue;
            const uint8_t *h = (const uint8_t *)dgram + off[i];
            uint32_t fo = 0;
            st[i] |= txf::l4_fields(h[9], ((uint32_t)h[6] << 8) | h[7], len[i] - (h[0] & 0x0fu) * 4u,
                                    first[i + 1] > first[i], flags, &fo);
        }
    }
    const int64_t r = run_host(mode, (const uint8_t *)dgram, off, len, reinterpret_cast<const uint8_t *>(l2), mss, n, mtu,
                               flags, first.data(), (uint8_t *)out, slot, flen);
    if (r >= 0 && status) std::memcpy(status, st.data(), n * 4);
    return r;
}

// The device plan of nstack_txf.h, or (tso: with mss, device memory or null) of nstack_tso.h.
int plan_dev(bool tso, const uint16_t *mss, const void *dgram, uint64_t dgram_bytes, const uint64_t *off,
             const uint32_t *len, uint64_t n, uint32_t mtu, uint32_t flags, uint32_t *status, uint64_t *first,
             void *stream) {
    int rc = check_call(mtu, flags, tso ? txf::kKnownFlagsTso : txf::kKnownFlags);
    if (rc) return rc;
    if (!first || (n && (!dgram || !off || !len))) return fcs::set_error(EINVAL, "null pointer");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPTRY(hipMemsetAsync(first, 0, 8, st), "zeroing the total");
        return 0;
    }
    txf::FParams p{};
    p.dg = (uint64_t)dgram;
    p.lo4 = floor4(p.dg);
    p.hi4 = ceil4(p.dg + dgram_bytes);
    p.off = off;
    p.len = len;
    p.n = n;
    p.mtu = mtu;
    p.flags = flags;
    p.mss = mss;
    // the block totals: scratch that lives on the stream, between the three launches
    return with_stream_scratch(plan::plan_blocks(n) * 8, st, [&](void *mem) {
        return (tso ? txf::launch_plan_tso : txf::launch_plan)(p, status, first, (uint64_t *)mem, st);
    });
}

}  // namespace

extern "C" {

uint32_t ether_tx_frame_count(uint32_t D, uint32_t hlen, uint32_t mtu) { return txf::frame_count(D, hlen, mtu); }

int ether_tx_frame_plan_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t mtu, uint32_t flags, uint32_t *status, uint64_t *first,
                            void *stream) {
    return plan_dev(false, nullptr, dgram, dgram_bytes, off, len, n, mtu, flags, status, first, stream);
}

int ether_tx_frame_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, const uint64_t *first,
                       void *out, uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status, uint32_t *fcs_out,
                       void *stream) {
    return frame_dev(Mode::kPlain, nullptr, dgram, dgram_bytes, off, len, l2, n, mtu, flags, first, out, slot, slots, flen, status, fcs_out,
                     stream);
}

int64_t ether_tx_frame_host(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                            const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, void *out,
                            uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status) {
    return frame_host(Mode::kPlain, nullptr, dgram, dgram_bytes, off, len, l2, n, mtu, flags, out, slot, slots, flen, status);
}

// The kernel the last frame-building launch of this process launched.
int fcs_debug_txf_last_launch(char *out, uint64_t cap) { return copy_name(route_name(txf::last_launch()), out, cap); }

// ---- include/nstack_txd.h ----
int ip_tx_frame_l4_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, const uint64_t *first,
                       void *out, uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status, uint32_t *fcs_out,
                       void *stream) {
    return frame_dev(Mode::kL4, nullptr, dgram, dgram_bytes, off, len, l2, n, mtu, flags, first, out, slot, slots, flen, status, fcs_out,
                     stream);
}

int64_t ip_tx_frame_l4_host(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                            const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, void *out,
                            uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status) {
    return frame_host(Mode::kL4, nullptr, dgram, dgram_bytes, off, len, l2, n, mtu, flags, out, slot, slots, flen, status);
}

int fcs_debug_txd_last_launch(char *out, uint64_t cap) { return copy_name(route_name(txf::last_launch_l4()), out, cap); }

// ---- include/nstack_tso.h ----
uint32_t ip_tx_tso_count(uint32_t D, uint32_t hlen, uint32_t thl, uint32_t tcp_flags, uint32_t ip_foff, uint32_t mss,
                         uint32_t mtu) {
    return txf::tso_count(D, hlen, thl, tcp_flags, ip_foff, mss, mtu);
}

int ip_tx_tso_plan_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags, uint32_t *status, uint64_t *first,
                       void *stream) {
    return plan_dev(true, mss, dgram, dgram_bytes, off, len, n, mtu, flags, status, first, stream);
}

int ip_tx_tso_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                  const struct txf_l2 *l2, const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags,
                  const uint64_t *first, void *out, uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status,
                  uint32_t *fcs_out, void *stream) {
    return frame_dev(Mode::kTso, mss, dgram, dgram_bytes, off, len, l2, n, mtu, flags, first, out, slot, slots, flen, status,
                     fcs_out, stream);
}

int64_t ip_tx_tso_host(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const struct txf_l2 *l2, const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags, void *out,
                       uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status) {
    return frame_host(Mode::kTso, mss, dgram, dgram_bytes, off, len, l2, n, mtu, flags, out, slot, slots, flen, status);
}

int fcs_debug_tso_last_launch(char *out, uint64_t cap) { return copy_name(route_name(txf::last_launch_tso()), out, cap); }

}  // extern "C"
