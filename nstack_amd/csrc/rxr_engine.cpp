// rxr_engine.cpp — the C ABI of include/nstack_rxr.h, include/nstack_rxd.h and include/nstack_gro.h
// around rxr_kernel.hip and gro_kernel.hip.
//
// Device forms validate and launch; the device plan takes its scratch from hipMallocAsync on the
// caller's stream. The host form plans on the host (rxr_plan.hpp), checks every frame and the
// capacity, and then runs the double-buffered H2D -> kernel -> D2H pipeline of host_pipe.hpp over
// datagram ranges on the engine's first GPU, in staging and with a cut of its own: a chunk is a run
// of consecutive datagrams; the frames that carry them are gathered back to back (their first
// 14 + ip_len bytes: padding and trailer stay behind), the chunk's contiguous output range comes
// back and its datagrams are copied into the caller's arena one by one. Frames that belong to no
// delivered datagram never travel. No CPU path: a failure is returned, never answered on the host,
// and the FCS engine's host-batch and fallback counters are not touched. The forms of nstack_rxd.h are
// the same calls with the summing build and the verdict launch behind it (an L4 request: null for the
// plain forms); the host form brings a chunk's verdict words back with its datagrams. The forms of
// nstack_gro.h are those of nstack_rxd.h with the coalescing plan, build and finishing launch.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstring>
#include <vector>

#include "../../include/nstack_gro.h"
#include "../../include/nstack_rxd.h"
#include "../../include/nstack_rxr.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "gro_launch.hpp"
#include "host_pipe.hpp"
#include "rxr_launch.hpp"

using namespace hostpipe;

namespace {

int check_call(uint32_t flags, uint32_t align, uint64_t n) {
    if (flags & ~rxr::kKnownFlags) return fcs::set_error(EINVAL, "unknown flag bits 0x%x", flags & ~rxr::kKnownFlags);
    if (rxr::check_geometry(flags, align)) return fcs::set_error(EINVAL, "align %u is no power of two in 1..128", align);
    if (n >= rxr::kMaxFrames)
        return fcs::set_error(EINVAL, "%llu frames: a batch holds fewer than %llu", (unsigned long long)n,
                              (unsigned long long)rxr::kMaxFrames);
    return 0;
}

// What every plan call checks, host or device.
int check_plan(uint32_t flags, uint32_t align, uint64_t n, const void *arena, const uint64_t *off, const uint32_t *len,
               const uint32_t *fstat, const uint64_t *dst, const uint32_t *dgi, const uint64_t *doff, const uint32_t *dlen) {
    const int rc = check_call(flags, align, n);
    if (rc) return rc;
    if (!doff || (n && (!arena || !off || !len || !fstat || !dst || !dgi || !dlen))) return fcs::set_error(EINVAL, "null pointer");
    return 0;
}

// launch_build with the work counter its rows take their frames from, leased from the FCS engine's
// ring of device `dev` for this launch. With p.dverdict (nstack_rxd.h): the accumulators and *bad are
// zeroed on the stream in front of the build, and the verdict launch follows it.
int launch(rxr::RParams &p, int dev, int cus, hipStream_t st) {
    if (p.dverdict) {
        HIPTRY(hipMemsetAsync(p.dverdict, 0, p.n * 4, st), "zeroing the datagram accumulators");
        if (p.bad) HIPTRY(hipMemsetAsync(p.bad, 0, 8, st), "zeroing the bad count");
    }
    const int rc = fcs::launch_with_counter(dev, (void *)st, [&](unsigned long long *ctr) -> int {
        p.ctr = ctr;
        HIPTRY(rxr::launch_build(p, cus, st), "launching the rxr kernel");
        return 0;
    });
    if (rc || !p.dverdict) return rc;
    HIPTRY(rxr::launch_verdict(p, st), "launching the rxd verdict kernel");
    return 0;
}

void set_arena(rxr::RParams &p, const void *arena, uint64_t arena_bytes) {
    p.base = (uint64_t)arena;
    p.arena_bytes = arena_bytes;
    p.lo4 = floor4(p.base);
    p.hi4 = ceil4(p.base + arena_bytes);
}

// ---- host pipeline ----
constexpr uint64_t kInBytes = 32ull << 20;     // a chunk's gathered frames
constexpr uint64_t kOutBytes = 32ull << 20;    // a chunk's datagrams with their alignment gaps
constexpr uint64_t kChunkDgs = 1ull << 16;
constexpr uint64_t kChunkFrames = 1ull << 18;
constexpr int kDepth = 2;
// One datagram always fits a chunk: it is at most 65535 bytes (+ 127 of gap), reassembled from at
// most 8190 frames of 14 + 60 gathered header bytes each whose payloads add up to at most 65515
// bytes, or merged (nstack_gro.h) from at most 32768 members of 14 + 60 + 60 gathered header bytes
// each whose payloads add up to less than 65535 bytes.
static_assert(8190ull * 74 + 65535 <= kInBytes && 65535 + 127 <= kOutBytes && 8190 <= kChunkFrames, "a datagram fits a chunk");
static_assert(gro::kMaxMembers * 134ull + 65535 <= kInBytes && gro::kMaxMembers <= kChunkFrames, "a merged datagram fits a chunk");

struct RxrPipe;   // names this engine's pipelines (host_pipe.hpp)
thread_local ChunkLog t_chunks;   // the datagrams of each chunk of this thread's last host call (tests)
enum { kIn, kOff, kLen, kStat, kDst, kDgi, kDoff, kDlen, kOut, kVerd, kCnt };
const std::vector<BufSpec> kBufs = {{kInBytes + 64, "rxr staging"}, {kChunkFrames * 8, "off"},  {kChunkFrames * 4, "len"},
                                    {kChunkFrames * 4, "fstat"},    {kChunkFrames * 8, "dst"},  {kChunkFrames * 4, "dgi"},
                                    {(kChunkDgs + 1) * 8, "doff"},  {kChunkDgs * 4, "dlen"},    {kOutBytes, "rxr datagrams"},
                                    {kChunkFrames * 4, "dverdict"}, {16, "counts"}};   // nstack_rxd.h: one word per frame of the chunk

// The host plan of the batch and, from it, the frames of every datagram in frame order.
struct HostPlan {
    std::vector<uint32_t> fstat, dgi, dlen, dlead, glen;   // glen: the bytes of frame i that travel
    std::vector<uint64_t> dst, doff, first, frames;        // datagram k's frames: frames[first[k] .. first[k + 1])
    uint64_t m = 0;
};

// dverdict: null for the plain form; else the caller's verdict words (nstack_rxd.h), one per datagram.
// gro: the coalescing build and finishing launch (nstack_gro.h; hp is then gro::plan_batch's).
int64_t run_host(const uint8_t *arena, const uint64_t *off, const HostPlan &hp, uint8_t *out, uint32_t *dverdict, bool gro) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    const uint64_t m = hp.m;
    auto span = [&](uint64_t k, uint64_t e) { return hp.doff[e - 1] + hp.dlen[e - 1] - hp.doff[k]; };   // bytes of datagrams [k, e)
    auto issue = [&](Slot &s, hipStream_t st, uint64_t k) -> int64_t {
        uint64_t e = k, sum = 0;
        while (e < m && e - k < kChunkDgs && hp.first[e + 1] - hp.first[k] <= kChunkFrames) {
            uint64_t g = 0;
            for (uint64_t q = hp.first[e]; q < hp.first[e + 1]; q++) g += hp.glen[hp.frames[q]];
            if (sum + g > kInBytes || span(k, e + 1) > kOutBytes) break;
            sum += g;
            e++;
        }
        if (e == k)   // a datagram always fits a chunk (above): cannot happen
            return fcs::set_error(EINVAL, "datagram %llu exceeds the host chunk", (unsigned long long)k);
        const uint64_t nd = e - k, nf = hp.first[e] - hp.first[k], base = hp.doff[k];
        t_chunks.add(nd);
        uint8_t *h_in = s.h<uint8_t>(kIn);
        uint64_t w = 0;
        for (uint64_t q = 0; q < nf; q++) {
            const uint64_t i = hp.frames[hp.first[k] + q];
            std::memcpy(h_in + w, arena + off[i], hp.glen[i]);
            s.h<uint64_t>(kOff)[q] = w;
            s.h<uint32_t>(kLen)[q] = hp.glen[i];
            s.h<uint32_t>(kStat)[q] = hp.fstat[i];
            s.h<uint64_t>(kDst)[q] = hp.dst[i] - base;
            s.h<uint32_t>(kDgi)[q] = hp.dgi[i] - (uint32_t)k;
            w += hp.glen[i];
        }
        for (uint64_t q = 0; q < nd; q++) {
            s.h<uint64_t>(kDoff)[q] = hp.doff[k + q] - base;
            s.h<uint32_t>(kDlen)[q] = hp.dlen[k + q];
        }
        const uint64_t ob = span(k, e);
        HIPTRY(hipMemcpyAsync(s.d<void>(kIn), h_in, w, hipMemcpyHostToDevice, st), "H2D frames");
        HIPTRY(hipMemcpyAsync(s.d<void>(kOff), s.h<void>(kOff), nf * 8, hipMemcpyHostToDevice, st), "H2D off");
        HIPTRY(hipMemcpyAsync(s.d<void>(kLen), s.h<void>(kLen), nf * 4, hipMemcpyHostToDevice, st), "H2D len");
        HIPTRY(hipMemcpyAsync(s.d<void>(kStat), s.h<void>(kStat), nf * 4, hipMemcpyHostToDevice, st), "H2D fstat");
        HIPTRY(hipMemcpyAsync(s.d<void>(kDst), s.h<void>(kDst), nf * 8, hipMemcpyHostToDevice, st), "H2D dst");
        HIPTRY(hipMemcpyAsync(s.d<void>(kDgi), s.h<void>(kDgi), nf * 4, hipMemcpyHostToDevice, st), "H2D dgi");
        HIPTRY(hipMemcpyAsync(s.d<void>(kDoff), s.h<void>(kDoff), nd * 8, hipMemcpyHostToDevice, st), "H2D doff");
        HIPTRY(hipMemcpyAsync(s.d<void>(kDlen), s.h<void>(kDlen), nd * 4, hipMemcpyHostToDevice, st), "H2D dlen");
        rxr::RParams p{};
        set_arena(p, s.d<void>(kIn), w);
        p.off = s.d<uint64_t>(kOff);
        p.len = s.d<uint32_t>(kLen);
        p.n = nf;
        p.flags = 0;   // the trailer stayed behind
        p.pstat = s.d<uint32_t>(kStat);
        p.dst = s.d<uint64_t>(kDst);
        p.dgi = s.d<uint32_t>(kDgi);
        p.doff = s.d<uint64_t>(kDoff);
        p.dlen = s.d<uint32_t>(kDlen);
        p.out = (uint64_t)s.d<void>(kOut);
        p.out_bytes = ob;
        if (dverdict) {   // the verdict launch reads the chunk's datagram count from device memory
            s.h<uint64_t>(kCnt)[0] = nd;
            s.h<uint64_t>(kCnt)[1] = ob;
            HIPTRY(hipMemcpyAsync(s.d<void>(kCnt), s.h<void>(kCnt), 16, hipMemcpyHostToDevice, st), "H2D counts");
            p.counts = s.d<uint64_t>(kCnt);
            p.dverdict = s.d<uint32_t>(kVerd);
            p.bad_mask = 0;   // bad is counted on the host
            p.gro = gro ? 1u : 0u;
        }
        if ((rc = launch(p, dev, cus, st))) return rc;
        HIPTRY(hipMemcpyAsync(s.h<void>(kOut), s.d<void>(kOut), ob, hipMemcpyDeviceToHost, st), "D2H datagrams");
        if (dverdict) HIPTRY(hipMemcpyAsync(s.h<void>(kVerd), s.d<void>(kVerd), nd * 4, hipMemcpyDeviceToHost, st), "D2H verdicts");
        s.i0 = k;   // the chunk's first datagram and their number
        s.n = nd;
        s.live = true;
        return (int64_t)e;
    };
    auto drain = [&](Slot &s) {
        const uint64_t base = hp.doff[s.i0];
        for (uint64_t q = s.i0; q < s.i0 + s.n; q++)
            std::memcpy(out + hp.doff[q], s.h<uint8_t>(kOut) + (hp.doff[q] - base), hp.dlen[q]);
        if (dverdict) std::memcpy(dverdict + s.i0, s.h<uint32_t>(kVerd), s.n * 4);
    };
    rc = run_pipe<RxrPipe>(dev, kDepth, kBufs, m, issue, drain);
    return rc ? (int64_t)rc : (int64_t)m;
}

// The device build of the three headers. l4: the form of nstack_rxd.h, which needs counts and
// dverdict; gro (with l4): that of nstack_gro.h.
int build_dev(bool l4, bool gro, const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
              uint32_t flags, const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi, const uint64_t *doff,
              const uint32_t *dlen, const uint64_t *counts, void *out, uint64_t out_bytes, uint32_t *fstat,
              uint32_t bad_mask, uint32_t *dverdict, uint64_t *bad, void *stream) {
    int rc = check_call(flags, 1u, n);
    if (rc) return rc;
    if (n && (!arena || !off || !len || !pstat || !dst || !dgi || !doff || !dlen || (!out && out_bytes)))
        return fcs::set_error(EINVAL, "null pointer");
    if (l4 && !counts) return fcs::set_error(EINVAL, "null counts: the verdict launch reads the datagram count there");
    if (l4 && n && !dverdict) return fcs::set_error(EINVAL, "null dverdict");
    if ((uint64_t)out + out_bytes < (uint64_t)out) return fcs::set_error(EINVAL, "out + out_bytes overflows");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        if (l4 && bad) HIPTRY(hipMemsetAsync(bad, 0, 8, st), "zeroing the bad count");
        return 0;
    }
    rxr::RParams p{};
    set_arena(p, arena, arena_bytes);
    p.off = off;
    p.len = len;
    p.n = n;
    p.flags = flags;
    p.pstat = pstat;
    p.dst = const_cast<uint64_t *>(dst);
    p.dgi = const_cast<uint32_t *>(dgi);
    p.doff = const_cast<uint64_t *>(doff);
    p.dlen = const_cast<uint32_t *>(dlen);
    p.out = (uint64_t)out;
    p.out_bytes = out_bytes;
    p.fstat = fstat;
    if (l4) {
        p.counts = const_cast<uint64_t *>(counts);
        p.dverdict = dverdict;
        p.bad = (unsigned long long *)bad;
        p.bad_mask = bad_mask;
        p.gro = gro ? 1u : 0u;
    }
    return launch(p, dev, cus, st);
}

// The device plan of nstack_rxr.h, or with gro that of nstack_gro.h.
int plan_dev(bool gro, const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
             uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat, uint64_t *dst,
             uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint64_t *counts, void *stream) {
    int rc = check_plan(flags, align, n, arena, off, len, fstat, dst, dgi, doff, dlen);
    if (rc) return rc;
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {
        HIPTRY(hipMemsetAsync(doff, 0, 8, st), "zeroing the total");
        if (counts) HIPTRY(hipMemsetAsync(counts, 0, 16, st), "zeroing the counts");
        return 0;
    }
    rxr::RParams p{};
    set_arena(p, arena, arena_bytes);
    p.off = off;
    p.len = len;
    p.n = n;
    p.flags = flags;
    p.align = align;
    p.verdict = verdict;
    p.drop_mask = drop_mask;
    p.fstat = fstat;
    p.dst = dst;
    p.dgi = dgi;
    p.doff = doff;
    p.dlen = dlen;
    p.dlead = dlead;
    p.counts = counts;
    // scratch that lives on the stream, between the launches
    const uint64_t rb = plan::up16(rxr::scratch_bytes(n));   // the coalescing plan's scratch lies behind
    return with_stream_scratch(gro ? rb + gro::scratch_bytes(n) : rxr::scratch_bytes(n), st, [&](void *mem) {
        hipError_t e = hipMemsetAsync(mem, 0, rxr::zeroed_bytes(n), st);
        if (e != hipSuccess) return e;
        if (!gro) return rxr::launch_plan(p, rxr::carve(mem, n), st);
        void *gmem = (uint8_t *)mem + rb;
        e = hipMemsetAsync(gmem, 0, gro::zeroed_bytes(n), st);
        return e == hipSuccess ? gro::launch_plan(p, rxr::carve(mem, n), gro::carve(gmem, n), st) : e;
    });
}

// A host plan call: the checks, then rxr::plan_batch, or with gro gro::plan_batch.
int64_t plan_host(bool gro, const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                  uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat, uint64_t *dst,
                  uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead) {
    const int rc = check_plan(flags, align, n, arena, off, len, fstat, dst, dgi, doff, dlen);
    if (rc) return rc;
    uint64_t bad = 0;
    const int64_t m = (gro ? gro::plan_batch : rxr::plan_batch)((const uint8_t *)arena, arena_bytes, off, len, n, flags, verdict,
                                                                drop_mask, align, fstat, dst, dgi, doff, dlen, dlead, &bad);
    if (m < 0)
        return fcs::set_error(EINVAL, "frame %llu [%llu, +%u) outside the %llu-byte arena", (unsigned long long)bad,
                              (unsigned long long)off[bad], len[bad], (unsigned long long)arena_bytes);
    return m;
}

// The host form of the three headers: dverdict is null for ether_rx_reasm_host; gro: nstack_gro.h.
int64_t reasm_host(bool gro, const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                   uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, void *out,
                   uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen, uint32_t *dlead,
                   uint32_t *dverdict) {
    t_chunks.clear();
    int rc = check_call(flags, align, n);
    if (rc) return rc;
    if (n == 0) {
        if (doff) doff[0] = 0;
        return 0;
    }
    if (!arena || !off || !len || (!out && out_bytes)) return fcs::set_error(EINVAL, "null pointer");
    HostPlan hp;
    hp.fstat.resize(n);
    hp.dgi.resize(n);
    hp.dlen.resize(n);
    hp.dlead.resize(n);
    hp.dst.resize(n);
    hp.doff.resize(n + 1);
    const int64_t m = plan_host(gro, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, hp.fstat.data(),
                                hp.dst.data(), hp.dgi.data(), hp.doff.data(), hp.dlen.data(), hp.dlead.data());
    if (m < 0) return m;
    hp.m = (uint64_t)m;
    const uint64_t need = hp.m ? hp.doff[hp.m - 1] + hp.dlen[hp.m - 1] : 0;   // rule 8: the last datagram's end
    if (need > out_bytes)
        return fcs::set_error(ENOSPC, "%llu datagrams need %llu bytes, more than the %llu given", (unsigned long long)hp.m,
                              (unsigned long long)need, (unsigned long long)out_bytes);
    // the frames of every datagram, in frame order (a counting sort by datagram), and what travels of each
    hp.first.assign(hp.m + 1, 0);
    hp.glen.assign(n, 0u);
    for (uint64_t i = 0; i < n; i++)
        if (hp.dgi[i] != rxr::kNone32) hp.first[hp.dgi[i] + 1]++;
    for (uint64_t k = 0; k < hp.m; k++) hp.first[k + 1] += hp.first[k];
    hp.frames.resize(hp.first[hp.m]);
    {
        std::vector<uint64_t> at(hp.first.begin(), hp.first.end() - 1);
        for (uint64_t i = 0; i < n; i++) {
            if (hp.dgi[i] == rxr::kNone32) continue;
            hp.frames[at[hp.dgi[i]]++] = i;
            const uint8_t *f = (const uint8_t *)arena + off[i];
            hp.glen[i] = 14u + (((uint32_t)f[16] << 8) | f[17]);   // 14 + ip_len <= F - T (rule 3)
        }
    }
    int dev = 0, cus = 0;   // no CPU path, also for a batch that delivers nothing
    if ((rc = fcs::engine_device0(&dev, &cus))) return rc;
    int64_t r = (int64_t)hp.m;
    if (hp.m) r = run_host((const uint8_t *)arena, off, hp, (uint8_t *)out, dverdict, gro);
    if (r < 0) return r;
    for (uint64_t i = 0; i < n && fstat; i++)
        fstat[i] = hp.fstat[i] | (hp.dgi[i] != rxr::kNone32 ? rxr::kDelivered : 0u);
    if (doff) std::memcpy(doff, hp.doff.data(), (hp.m + 1) * 8);
    if (dlen) std::memcpy(dlen, hp.dlen.data(), hp.m * 4);
    if (dlead) std::memcpy(dlead, hp.dlead.data(), hp.m * 4);
    return r;
}

// The host form of nstack_rxd.h and, with gro, of nstack_gro.h: reasm_host with the verdict words, and
// *bad counted on the host.
int64_t reasm_l4_host(bool gro, const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                      uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, void *out,
                      uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint32_t bad_mask,
                      uint32_t *dverdict, uint64_t *bad) {
    if (n && !dverdict) return fcs::set_error(EINVAL, "null dverdict");
    const int64_t m = reasm_host(gro, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, out, out_bytes, fstat,
                                 doff, dlen, dlead, dverdict);
    if (m < 0 || !bad) return m;
    *bad = 0;
    for (int64_t k = 0; k < m; k++) *bad += (dverdict[k] & bad_mask) != 0u;
    return m;
}

}  // namespace

extern "C" {

int64_t ether_rx_reasm_plan_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                                 uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask,
                                 uint32_t align, uint32_t *fstat, uint64_t *dst, uint32_t *dgi, uint64_t *doff,
                                 uint32_t *dlen, uint32_t *dlead) {
    return plan_host(false, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, fstat, dst, dgi, doff, dlen, dlead);
}

int ether_rx_reasm_plan_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align,
                            uint32_t *fstat, uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen,
                            uint32_t *dlead, uint64_t *counts, void *stream) {
    return plan_dev(false, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, fstat, dst, dgi, doff, dlen, dlead,
                    counts, stream);
}

int ether_rx_reasm_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi,
                       const uint64_t *doff, const uint32_t *dlen, void *out, uint64_t out_bytes, uint32_t *fstat,
                       void *stream) {
    return build_dev(false, false, arena, arena_bytes, off, len, n, flags, pstat, dst, dgi, doff, dlen, nullptr, out, out_bytes, fstat,
                     0u, nullptr, nullptr, stream);
}

int64_t ether_rx_reasm_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align,
                            void *out, uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen,
                            uint32_t *dlead) {
    return reasm_host(false, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, out, out_bytes, fstat, doff,
                      dlen, dlead, nullptr);
}

// ---- include/nstack_rxd.h ----
int ip_rx_reasm_l4_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi,
                       const uint64_t *doff, const uint32_t *dlen, const uint64_t *counts, void *out, uint64_t out_bytes,
                       uint32_t *fstat, uint32_t bad_mask, uint32_t *dverdict, uint64_t *bad, void *stream) {
    return build_dev(true, false, arena, arena_bytes, off, len, n, flags, pstat, dst, dgi, doff, dlen, counts, out, out_bytes, fstat,
                     bad_mask, dverdict, bad, stream);
}

int64_t ip_rx_reasm_l4_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align,
                            void *out, uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen,
                            uint32_t *dlead, uint32_t bad_mask, uint32_t *dverdict, uint64_t *bad) {
    return reasm_l4_host(false, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, out, out_bytes, fstat, doff, dlen,
                         dlead, bad_mask, dverdict, bad);
}

// ---- include/nstack_gro.h ----
int64_t ip_rx_gro_plan_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                            uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat,
                            uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead) {
    return plan_host(true, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, fstat, dst, dgi, doff, dlen, dlead);
}

int ip_rx_gro_plan_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat,
                       uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint64_t *counts,
                       void *stream) {
    return plan_dev(true, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, fstat, dst, dgi, doff, dlen, dlead,
                    counts, stream);
}

int ip_rx_gro_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n, uint32_t flags,
                  const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi, const uint64_t *doff, const uint32_t *dlen,
                  const uint64_t *counts, void *out, uint64_t out_bytes, uint32_t *fstat, uint32_t bad_mask,
                  uint32_t *dverdict, uint64_t *bad, void *stream) {
    return build_dev(true, true, arena, arena_bytes, off, len, n, flags, pstat, dst, dgi, doff, dlen, counts, out, out_bytes, fstat,
                     bad_mask, dverdict, bad, stream);
}

int64_t ip_rx_gro_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, void *out,
                       uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint32_t bad_mask,
                       uint32_t *dverdict, uint64_t *bad) {
    return reasm_l4_host(true, arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, out, out_bytes, fstat, doff, dlen,
                         dlead, bad_mask, dverdict, bad);
}

// The kernel the last coalescing build launch of this process launched.
int fcs_debug_gro_last_launch(char *out, uint64_t cap) {
    return copy_name(rxr::last_launch_gro() == rxr::Route::kGro ? "gro" : "none", out, cap);
}

// The kernel the last build launch with sums of this process launched.
int fcs_debug_rxd_last_launch(char *out, uint64_t cap) {
    return copy_name(rxr::last_launch_l4() == rxr::Route::kGeneralL4 ? "general-l4" : "none", out, cap);
}

// The kernel the last build launch of this process launched.
int fcs_debug_rxr_last_launch(char *out, uint64_t cap) {
    return copy_name(rxr::last_launch() == rxr::Route::kGeneral ? "general" : "none", out, cap);
}

int64_t fcs_debug_rxr_last_host_chunks(uint64_t *dgs, uint64_t cap) {
    return t_chunks.report(dgs, cap);
}

}  // extern "C"
