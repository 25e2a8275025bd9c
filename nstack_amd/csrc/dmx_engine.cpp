// dmx_engine.cpp — the C ABI of include/nstack_dmx.h around dmx_kernel.hip.
//
// Device forms validate and launch; the device plan takes its scratch from one hipMallocAsync on the
// caller's stream. The host form plans on the host (dmx_plan.hpp), checks the capacity, and then runs
// the double-buffered H2D -> kernel -> D2H pipeline of host_pipe.hpp over ranges of consecutive
// datagrams cut by host_chunk.hpp (a datagram that makes no record travels as zero bytes): the device
// builds a chunk's records back to back in k order into the slot, and on completion the host moves
// each record to q + rec[k]. No CPU path: a failure is returned, never answered on the host, and the
// FCS engine's host-batch and fallback counters are not touched.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstring>
#include <vector>

#include "../../include/nstack_dmx.h"
#include "dmx_launch.hpp"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_pipe.hpp"

using namespace hostpipe;

namespace {

int check_call(uint32_t align, uint64_t S, uint64_t n) {
    if (align < 8u || align > 128u || (align & (align - 1u)))
        return fcs::set_error(EINVAL, "align %u is no power of two in 8..128", align);
    if (dmx::check_geometry(align, S))
        return fcs::set_error(EINVAL, "%llu sockets: a bind table holds at most %u", (unsigned long long)S, dmx::kMaxSocks);
    if (n >= dmx::kMaxDgs)
        return fcs::set_error(EINVAL, "%llu datagrams: a batch holds fewer than %llu", (unsigned long long)n,
                              (unsigned long long)dmx::kMaxDgs);
    return 0;
}

int check_plan_args(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen, uint64_t n,
                    const uint64_t *bind, uint32_t S, const uint32_t *dstat, const uint32_t *dsock, const uint64_t *rec,
                    const uint64_t *sbase, const uint32_t *scnt) {
    if (!sbase || (S && (!bind || !scnt)) || (n && (!out || !doff || !dlen || !dstat || !dsock || !rec)))
        return fcs::set_error(EINVAL, "null pointer");
    if ((uint64_t)out + out_bytes < (uint64_t)out) return fcs::set_error(EINVAL, "out + out_bytes overflows");
    return 0;
}

int64_t plan_host(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen, const uint32_t *dverdict,
                  uint64_t n, const uint64_t *bind, uint32_t S, uint32_t drop_mask, uint32_t align, uint32_t *dstat,
                  uint32_t *dsock, uint64_t *rec, uint64_t *sbase, uint32_t *scnt) {
    uint64_t bad = 0;
    const int64_t r = dmx::plan_batch((const uint8_t *)out, out_bytes, doff, dlen, dverdict, n, bind, S, drop_mask, align, dstat,
                                      dsock, rec, sbase, scnt, &bad);
    if (r < 0)
        return fcs::set_error(EINVAL, "bind key %llu is 0x%016llx: proto is neither 6 nor 17, or bits 56..63 are set",
                              (unsigned long long)bad, (unsigned long long)bind[bad]);
    return r;
}

// ---- host pipeline ----
constexpr uint64_t kInBytes = 32ull << 20;     // a chunk's datagrams
constexpr uint64_t kChunkDgs = 1ull << 16;
// A record is its datagram without the 28 header bytes at the least, plus 24 and less than 128 of pad.
constexpr uint64_t kOutBytes = kInBytes + kChunkDgs * 124;
constexpr int kDepth = 2;
static_assert(65535 <= kInBytes, "a datagram fits a chunk");
static_assert(dmx::kRecHdr + 127 - 28 <= 124, "a chunk's records fit its output buffer");

struct DmxPipe;   // names this engine's pipelines (host_pipe.hpp)
thread_local ChunkLog t_chunks;   // the datagrams of each chunk of this thread's last host call (tests)
enum { kIn, kOff, kLen, kStat, kRec, kOut, kCnt };   // host_pipe.hpp's stage_h2d wants frames, offsets and lengths first
const std::vector<BufSpec> kBufs = {{kInBytes + 64, "dmx staging"}, {kChunkDgs * 8, "doff"},   {kChunkDgs * 4, "dlen"},
                                    {kChunkDgs * 4, "pstat"},       {kChunkDgs * 8, "rec"},    {kOutBytes, "dmx records"},
                                    {16, "counts"}};

struct HostPlan {
    std::vector<uint32_t> dstat, dsock, scnt, glen, size;   // glen: the bytes of datagram k that travel; size: its record's
    std::vector<uint64_t> rec, sbase, goff;
};

int run_host(const uint8_t *out, uint64_t n, const HostPlan &hp, uint32_t align, uint8_t *q) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    auto issue = [&](Slot &s, hipStream_t st, uint64_t i) -> int64_t {
        const hostchunk::Cut c = hostchunk::cut(hp.goff.data(), hp.glen.data(), i, n, kInBytes, kChunkDgs, 0);
        if (c.e == i)   // a datagram always fits a chunk (above): cannot happen
            return fcs::set_error(EINVAL, "datagram %llu exceeds the host chunk", (unsigned long long)i);
        const uint64_t np = c.e - i;
        t_chunks.add(np);
        uint64_t ob = 0;
        for (uint64_t x = 0; x < np; x++) {
            const bool queued = hp.dstat[i + x] & dmx::kQueued;
            s.h<uint32_t>(kStat)[x] = hp.dstat[i + x];
            s.h<uint64_t>(kRec)[x] = queued ? ob : dmx::kNone64;
            ob += hp.size[i + x];
        }
        s.i0 = i;
        s.n = np;
        if (ob == 0) return (int64_t)c.e;   // no record in the chunk: no device work
        int r2 = stage_h2d(s, st, out, hp.goff.data(), hp.glen.data(), i, c, kInBytes, 0, "H2D datagrams");
        if (r2) return r2;
        const uint64_t span = hostchunk::dense(c, kInBytes) ? (c.lo & 15) + (c.hi - c.lo) : c.sum;
        s.h<uint64_t>(kCnt)[0] = np;
        s.h<uint64_t>(kCnt)[1] = span;
        HIPTRY(hipMemcpyAsync(s.d<void>(kStat), s.h<void>(kStat), np * 4, hipMemcpyHostToDevice, st), "H2D pstat");
        HIPTRY(hipMemcpyAsync(s.d<void>(kRec), s.h<void>(kRec), np * 8, hipMemcpyHostToDevice, st), "H2D rec");
        HIPTRY(hipMemcpyAsync(s.d<void>(kCnt), s.h<void>(kCnt), 16, hipMemcpyHostToDevice, st), "H2D counts");
        dmx::DParams p{};
        p.out = (uint64_t)s.d<void>(kIn);
        p.out_bytes = span;
        p.doff = s.d<uint64_t>(kOff);
        p.dlen = s.d<uint32_t>(kLen);
        p.counts = s.d<uint64_t>(kCnt);
        p.n = np;
        p.align = align;
        p.pstat = s.d<uint32_t>(kStat);
        p.rec = s.d<uint64_t>(kRec);
        p.q = (uint64_t)s.d<void>(kOut);
        p.q_bytes = ob;
        r2 = fcs::launch_with_counter(dev, (void *)st, [&](unsigned long long *ctr) -> int {
            p.ctr = ctr;
            HIPTRY(dmx::launch_build(p, cus, st), "launching the dmx kernel");
            return 0;
        });
        if (r2) return r2;
        HIPTRY(hipMemcpyAsync(s.h<void>(kOut), s.d<void>(kOut), ob, hipMemcpyDeviceToHost, st), "D2H records");
        s.live = true;
        return (int64_t)c.e;
    };
    auto drain = [&](Slot &s) {
        uint64_t at = 0;
        for (uint64_t k = s.i0; k < s.i0 + s.n; k++) {
            if (hp.size[k]) std::memcpy(q + hp.rec[k], s.h<uint8_t>(kOut) + at, hp.size[k]);
            at += hp.size[k];
        }
    };
    return run_pipe<DmxPipe>(dev, kDepth, kBufs, n, issue, drain);
}

}  // namespace

extern "C" {

int64_t ip_rx_demux_plan_host(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                              const uint32_t *dverdict, uint64_t n, const uint64_t *bind, uint32_t S, uint32_t drop_mask,
                              uint32_t align, uint32_t *dstat, uint32_t *dsock, uint64_t *rec, uint64_t *sbase, uint32_t *scnt) {
    int rc = check_call(align, S, n);
    if (rc) return rc;
    if ((rc = check_plan_args(out, out_bytes, doff, dlen, n, bind, S, dstat, dsock, rec, sbase, scnt))) return rc;
    return plan_host(out, out_bytes, doff, dlen, dverdict, n, bind, S, drop_mask, align, dstat, dsock, rec, sbase, scnt);
}

int ip_rx_demux_plan_dev(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                         const uint32_t *dverdict, const uint64_t *counts, uint64_t n, const uint64_t *bind, uint32_t S,
                         uint32_t drop_mask, uint32_t align, uint32_t *dstat, uint32_t *dsock, uint64_t *rec, uint64_t *sbase,
                         uint32_t *scnt, uint64_t *qcounts, void *stream) {
    int rc = check_call(align, S, n);
    if (rc) return rc;
    if ((rc = check_plan_args(out, out_bytes, doff, dlen, n, bind, S, dstat, dsock, rec, sbase, scnt))) return rc;
    if (!qcounts) return fcs::set_error(EINVAL, "null qcounts");
    if (n && !counts) return fcs::set_error(EINVAL, "null counts: the plan reads the datagram count there");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPTRY(hipMemsetAsync(qcounts, 0, 32, st), "zeroing qcounts");
    if (n == 0) {
        HIPTRY(hipMemsetAsync(sbase, 0, ((uint64_t)S + 1) * 8, st), "zeroing sbase");
        if (S) HIPTRY(hipMemsetAsync(scnt, 0, (uint64_t)S * 4, st), "zeroing scnt");
        return 0;
    }
    dmx::DParams p{};
    p.out = (uint64_t)out;
    p.out_bytes = out_bytes;
    p.doff = doff;
    p.dlen = dlen;
    p.dverdict = dverdict;
    p.counts = counts;
    p.n = n;
    p.bind = bind;
    p.S = S;
    p.drop_mask = drop_mask;
    p.align = align;
    p.dstat = dstat;
    p.dsock = dsock;
    p.rec = rec;
    p.sbase = sbase;
    p.scnt = scnt;
    p.qcounts = qcounts;
    // scratch that lives on the stream, between the launches
    return with_stream_scratch(dmx::scratch_bytes(n, S), st, [&](void *mem) {
        hipError_t e = hipMemsetAsync(mem, 0, dmx::zero_bytes(S), st);
        if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)mem + dmx::zero_bytes(S), 0xff, dmx::ones_bytes(n, S), st);
        return e == hipSuccess ? dmx::launch_plan(p, dmx::carve(mem, n, S), st) : e;
    });
}

int ip_rx_demux_dev(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen, const uint64_t *counts,
                    uint64_t n, const uint32_t *pstat, const uint64_t *rec, uint32_t align, void *q, uint64_t q_bytes,
                    uint32_t *dstat, void *stream) {
    int rc = check_call(align, 0, n);
    if (rc) return rc;
    if (n && (!out || !doff || !dlen || !counts || !pstat || !rec || (!q && q_bytes))) return fcs::set_error(EINVAL, "null pointer");
    if ((uint64_t)out + out_bytes < (uint64_t)out) return fcs::set_error(EINVAL, "out + out_bytes overflows");
    if ((uint64_t)q + q_bytes < (uint64_t)q) return fcs::set_error(EINVAL, "q + q_bytes overflows");
    if ((uint64_t)q & (align - 1u)) return fcs::set_error(EINVAL, "q is not aligned to %u", align);
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    dmx::DParams p{};
    p.out = (uint64_t)out;
    p.out_bytes = out_bytes;
    p.doff = doff;
    p.dlen = dlen;
    p.counts = counts;
    p.n = n;
    p.align = align;
    p.pstat = pstat;
    p.rec = const_cast<uint64_t *>(rec);
    p.q = (uint64_t)q;
    p.q_bytes = q_bytes;
    p.dstat = dstat;
    return fcs::launch_with_counter(dev, (void *)st, [&](unsigned long long *ctr) -> int {
        p.ctr = ctr;
        HIPTRY(dmx::launch_build(p, cus, st), "launching the dmx kernel");
        return 0;
    });
}

int64_t ip_rx_demux_host(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                         const uint32_t *dverdict, uint64_t n, const uint64_t *bind, uint32_t S, uint32_t drop_mask,
                         uint32_t align, void *q, uint64_t q_bytes, uint32_t *dstat, uint32_t *dsock, uint64_t *rec,
                         uint64_t *sbase, uint32_t *scnt) {
    t_chunks.clear();
    int rc = check_call(align, S, n);
    if (rc) return rc;
    if ((S && !bind) || (n && (!out || !doff || !dlen)) || (!q && q_bytes)) return fcs::set_error(EINVAL, "null pointer");
    if ((uint64_t)out + out_bytes < (uint64_t)out) return fcs::set_error(EINVAL, "out + out_bytes overflows");
    HostPlan hp;
    hp.dstat.resize(n);
    hp.dsock.resize(n);
    hp.rec.resize(n);
    hp.sbase.resize((size_t)S + 1);
    hp.scnt.resize(S);
    const int64_t records = plan_host(out, out_bytes, doff, dlen, dverdict, n, bind, S, drop_mask, align, hp.dstat.data(),
                                      hp.dsock.data(), hp.rec.data(), hp.sbase.data(), hp.scnt.data());
    if (records < 0) return records;
    if (hp.sbase[S] > q_bytes)   // rule 8: a record has no room
        return fcs::set_error(ENOSPC, "%lld records need %llu bytes, more than the %llu given", (long long)records,
                              (unsigned long long)hp.sbase[S], (unsigned long long)q_bytes);
    int dev = 0, cus = 0;   // no CPU path, also for a batch that queues nothing
    if ((rc = fcs::engine_device0(&dev, &cus))) return rc;
    if (records) {
        // what travels: the datagrams with a record; the others as zero bytes at the end of the one before
        hp.glen.assign(n, 0u);
        hp.size.assign(n, 0u);
        hp.goff.assign(n, 0ull);
        uint64_t last = 0;
        for (uint64_t k = 0; k < n; k++) {
            if (hp.dstat[k] & dmx::kQueued) {
                hp.glen[k] = dlen[k];
                hp.goff[k] = doff[k];
                last = doff[k] + dlen[k];
                const dmx::Cls c = dmx::classify(doff[k], dlen[k], out_bytes, false, [&](uint64_t i) { return ((const uint8_t *)out)[i]; });
                hp.size[k] = (uint32_t)dmx::rec_size(c.P, align);
            } else {
                hp.goff[k] = last;
            }
        }
        if ((rc = run_host((const uint8_t *)out, n, hp, align, (uint8_t *)q))) return rc;
    }
    for (uint64_t k = 0; k < n; k++) {
        if (dstat) dstat[k] = hp.dstat[k] | ((hp.dstat[k] & dmx::kQueued) ? dmx::kDelivered : 0u);
        if (dsock) dsock[k] = hp.dsock[k];
        if (rec) rec[k] = hp.rec[k];
    }
    if (sbase) std::memcpy(sbase, hp.sbase.data(), ((size_t)S + 1) * 8);
    if (scnt && S) std::memcpy(scnt, hp.scnt.data(), (size_t)S * 4);
    return records;
}

int fcs_debug_dmx_last_launch(char *out, uint64_t cap) {
    return copy_name(dmx::last_launch() == dmx::Route::kDemux ? "demux" : "none", out, cap);
}

int64_t fcs_debug_dmx_last_host_chunks(uint64_t *dgs, uint64_t cap) {
    return t_chunks.report(dgs, cap);
}

}  // extern "C"
