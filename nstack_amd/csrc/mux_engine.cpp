// mux_engine.cpp — the C ABI of include/nstack_mux.h around mux_kernel.hip.
//
// Device forms validate and launch; the device plan takes its scratch from one hipMallocAsync on the
// caller's stream. The host form plans on the host (mux_plan.hpp), checks the capacity, and then runs
// the double-buffered H2D -> kernel -> D2H pipeline of host_pipe.hpp over ranges of consecutive
// records cut by host_chunk.hpp (a record that makes no datagram travels as zero bytes): a chunk's
// records are gathered on 16-byte starts into the slot, the device builds its datagrams back to back
// in k order, and on completion the host moves each datagram to dgram + off[k]. No CPU path: a
// failure is returned, never answered on the host, and the FCS engine's host-batch and fallback
// counters are not touched.
#include <hip/hip_runtime.h>

#include <cerrno>
#include <cstring>
#include <vector>

#include "../../include/nstack_mux.h"
#include "fcs_device.hpp"
#include "fcs_error.hpp"
#include "host_pipe.hpp"
#include "mux_launch.hpp"

using namespace hostpipe;

namespace {

int check_call(uint32_t align, uint64_t S, uint64_t R, uint64_t N, uint64_t n) {
    if (align < 4u || align > 128u || (align & (align - 1u)))
        return fcs::set_error(EINVAL, "align %u is no power of two in 4..128", align);
    if (S > mux::kMaxSocks) return fcs::set_error(EINVAL, "%llu sockets: a batch holds at most %u", (unsigned long long)S, mux::kMaxSocks);
    if (R > mux::kMaxRoutes) return fcs::set_error(EINVAL, "%llu routes: a route table holds at most %u", (unsigned long long)R, mux::kMaxRoutes);
    if (N > mux::kMaxNeigh)
        return fcs::set_error(EINVAL, "%llu neighbours: a neighbour table holds at most %u", (unsigned long long)N, mux::kMaxNeigh);
    if (n >= mux::kMaxRecs)
        return fcs::set_error(EINVAL, "%llu records: a batch holds fewer than %llu", (unsigned long long)n, (unsigned long long)mux::kMaxRecs);
    if (n && !S) return fcs::set_error(EINVAL, "%llu records and no socket", (unsigned long long)n);
    return 0;
}

int check_inputs(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst, const uint64_t *bind,
                 uint32_t S, const void *rt, uint32_t R, const void *nb, uint32_t N) {
    if ((S && (!bind || !sfirst)) || (R && !rt) || (N && !nb) || (n && (!q || !rec))) return fcs::set_error(EINVAL, "null pointer");
    if ((uint64_t)q + q_bytes < (uint64_t)q) return fcs::set_error(EINVAL, "q + q_bytes overflows");
    return 0;
}

int check_sfirst(const uint64_t *sfirst, uint32_t S, uint64_t n) {
    if (!mux::sfirst_ok(sfirst, S, n))
        return fcs::set_error(EINVAL, "sfirst is not monotone from 0 to n = %llu over %u sockets", (unsigned long long)n, S);
    return 0;
}

// ---- host pipeline ----
constexpr uint64_t kInBytes = 32ull << 20;     // a chunk's records
constexpr uint64_t kChunkRecs = 1ull << 16;
constexpr uint64_t kStageBytes = kInBytes + kChunkRecs * 16;   // each record is gathered on a 16-byte start
// A datagram is its record plus the 16 bytes by which a TCP header exceeds the record's, on a 4-byte start.
constexpr uint64_t kOutBytes = kInBytes + kChunkRecs * 20;
constexpr int kDepth = 2;
static_assert(mux::kRecHdr + mux::kTcpMax <= kInBytes && mux::kRecHdr + mux::kUdpMax <= kInBytes, "a record fits a chunk");
static_assert(40 - mux::kRecHdr + 3 <= 20, "a chunk's datagrams fit its output buffer");

struct MuxPipe;   // names this engine's pipelines (host_pipe.hpp)
thread_local ChunkLog t_chunks;   // the records of each chunk of this thread's last host call (tests)
enum { kIn, kRec, kStat, kOff, kLen, kHimg, kOut };
const std::vector<BufSpec> kBufs = {{kStageBytes, "mux staging"}, {kChunkRecs * 8, "rec"},  {kChunkRecs * 4, "pstat"},
                                    {kChunkRecs * 8, "off"},      {kChunkRecs * 4, "len"},  {kChunkRecs * mux::kImg, "himg"},
                                    {kOutBytes, "mux datagrams"}};

struct HostPlan {
    std::vector<uint32_t> mstat, len, tnext, glen;   // glen: the bytes of record k that travel
    std::vector<uint64_t> off, goff;
    std::vector<txf_l2> l2;
    std::vector<uint8_t> himg;
    uint64_t counts[4] = {0, 0, 0, 0};
};

int run_host(const uint8_t *q, const uint64_t *rec, uint64_t n, const HostPlan &hp, uint8_t *dgram) {
    int dev = 0, cus = 0;
    int rc = fcs::engine_device0(&dev, &cus);
    if (rc) return rc;
    auto issue = [&](Slot &s, hipStream_t st, uint64_t i) -> int64_t {
        const hostchunk::Cut c = hostchunk::cut(hp.goff.data(), hp.glen.data(), i, n, kInBytes, kChunkRecs, 0);
        if (c.e == i)   // a record always fits a chunk (above): cannot happen
            return fcs::set_error(EINVAL, "record %llu exceeds the host chunk", (unsigned long long)i);
        const uint64_t np = c.e - i;
        t_chunks.add(np);
        uint64_t ib = 0, ob = 0;
        for (uint64_t x = 0; x < np; x++) {
            const uint64_t k = i + x;
            s.h<uint32_t>(kStat)[x] = hp.mstat[k];
            s.h<uint64_t>(kRec)[x] = ib;
            s.h<uint64_t>(kOff)[x] = ob;
            s.h<uint32_t>(kLen)[x] = hp.len[k];
            if (hp.glen[k]) {
                std::memcpy(s.h<uint8_t>(kIn) + ib, q + rec[k], hp.glen[k]);
                ib += (hp.glen[k] + 15ull) & ~15ull;
                ob += ceil4(hp.len[k]);
            }
        }
        s.i0 = i;
        s.n = np;
        if (ob == 0) return (int64_t)c.e;   // no datagram in the chunk: no device work
        std::memcpy(s.h<uint8_t>(kHimg), hp.himg.data() + i * mux::kImg, np * mux::kImg);
        HIPTRY(hipMemcpyAsync(s.d<void>(kIn), s.h<void>(kIn), ib, hipMemcpyHostToDevice, st), "H2D records");
        HIPTRY(hipMemcpyAsync(s.d<void>(kRec), s.h<void>(kRec), np * 8, hipMemcpyHostToDevice, st), "H2D rec");
        HIPTRY(hipMemcpyAsync(s.d<void>(kStat), s.h<void>(kStat), np * 4, hipMemcpyHostToDevice, st), "H2D pstat");
        HIPTRY(hipMemcpyAsync(s.d<void>(kOff), s.h<void>(kOff), np * 8, hipMemcpyHostToDevice, st), "H2D off");
        HIPTRY(hipMemcpyAsync(s.d<void>(kLen), s.h<void>(kLen), np * 4, hipMemcpyHostToDevice, st), "H2D len");
        HIPTRY(hipMemcpyAsync(s.d<void>(kHimg), s.h<void>(kHimg), np * mux::kImg, hipMemcpyHostToDevice, st), "H2D himg");
        mux::MParams p{};
        p.q = (uint64_t)s.d<void>(kIn);
        p.q_bytes = ib;
        p.rec = s.d<uint64_t>(kRec);
        p.n = np;
        p.align = 4u;   // inside the slot; the caller's align is in hp.off
        p.pstat = s.d<uint32_t>(kStat);
        p.off = s.d<uint64_t>(kOff);
        p.len = s.d<uint32_t>(kLen);
        p.himg = s.d<uint32_t>(kHimg);
        p.dgram = (uint64_t)s.d<void>(kOut);
        p.dgram_bytes = ob;
        int r2 = fcs::launch_with_counter(dev, (void *)st, [&](unsigned long long *ctr) -> int {
            p.ctr = ctr;
            HIPTRY(mux::launch_build(p, cus, st), "launching the mux kernel");
            return 0;
        });
        if (r2) return r2;
        HIPTRY(hipMemcpyAsync(s.h<void>(kOut), s.d<void>(kOut), ob, hipMemcpyDeviceToHost, st), "D2H datagrams");
        s.live = true;
        return (int64_t)c.e;
    };
    auto drain = [&](Slot &s) {
        uint64_t at = 0;
        for (uint64_t k = s.i0; k < s.i0 + s.n; k++) {
            if (!hp.glen[k]) continue;
            std::memcpy(dgram + hp.off[k], s.h<uint8_t>(kOut) + at, hp.len[k]);
            at += ceil4(hp.len[k]);
        }
    };
    return run_pipe<MuxPipe>(dev, kDepth, kBufs, n, issue, drain);
}

void fill_params(mux::MParams &p, const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n) {
    p.q = (uint64_t)q;
    p.q_bytes = q_bytes;
    p.rec = rec;
    p.n = n;
}

}  // namespace

extern "C" {

int64_t ip_tx_mux_plan_host(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                            const uint64_t *bind, uint32_t S, const struct mux_tcb *tcb, const struct mux_route *rt, uint32_t R,
                            const struct mux_neigh *nb, uint32_t N, uint32_t id0, uint32_t align, uint32_t *mstat, uint64_t *off,
                            uint32_t *len, struct txf_l2 *l2, void *himg, uint32_t *tnext, uint64_t *counts) {
    int rc = check_call(align, S, R, N, n);
    if (rc) return rc;
    if ((rc = check_inputs(q, q_bytes, rec, n, sfirst, bind, S, rt, R, nb, N))) return rc;
    if (n && (!mstat || !off || !len || !l2 || !himg)) return fcs::set_error(EINVAL, "null pointer");
    if ((rc = check_sfirst(sfirst, S, n))) return rc;
    return mux::plan_batch((const uint8_t *)q, q_bytes, rec, n, sfirst, bind, S, tcb, rt, R, nb, N, id0, align, mstat, off, len, l2,
                           (uint8_t *)himg, tnext, counts);
}

int ip_tx_mux_plan_dev(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                       const uint64_t *bind, uint32_t S, const struct mux_tcb *tcb, const struct mux_route *rt, uint32_t R,
                       const struct mux_neigh *nb, uint32_t N, uint32_t id0, uint32_t align, uint32_t *mstat, uint64_t *off,
                       uint32_t *len, struct txf_l2 *l2, void *himg, uint32_t *tnext, uint64_t *counts, void *stream) {
    int rc = check_call(align, S, R, N, n);
    if (rc) return rc;
    if ((rc = check_inputs(q, q_bytes, rec, n, sfirst, bind, S, rt, R, nb, N))) return rc;
    if (n && (!mstat || !off || !len || !l2 || !himg)) return fcs::set_error(EINVAL, "null pointer");
    if (!counts) return fcs::set_error(EINVAL, "null counts");
    if ((uint64_t)q & 7u) return fcs::set_error(EINVAL, "q is not aligned to 8");
    if ((uint64_t)himg & 3u) return fcs::set_error(EINVAL, "himg is not aligned to 4");
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIPTRY(hipMemsetAsync(counts, 0, 32, st), "zeroing counts");
    if (n == 0 && !(S && tnext)) return 0;
    mux::MParams p{};
    fill_params(p, q, q_bytes, rec, n);
    p.sfirst = sfirst;
    p.bind = bind;
    p.tcb = tcb;
    p.rt = rt;
    p.nb = nb;
    p.S = S;
    p.R = R;
    p.N = N;
    p.id0 = id0;
    p.align = align;
    p.mstat = mstat;
    p.off = off;
    p.len = len;
    p.l2 = l2;
    p.himg = (uint32_t *)himg;
    p.tnext = tnext;
    p.counts = counts;
    // scratch that lives on the stream, between the launches
    return with_stream_scratch(mux::scratch_bytes(n, N), st, [&](void *mem) {
        hipError_t e = hipMemsetAsync(mem, 0, mux::zero_bytes(N), st);
        if (e == hipSuccess) e = hipMemsetAsync((uint8_t *)mem + mux::zero_bytes(N), 0xff, mux::ones_bytes(N), st);
        return e == hipSuccess ? mux::launch_plan(p, mux::carve(mem, n, N), st) : e;
    });
}

int ip_tx_mux_dev(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint32_t *pstat, const uint64_t *off,
                  const uint32_t *len, const void *himg, uint32_t align, void *dgram, uint64_t dgram_bytes, uint32_t *mstat,
                  void *stream) {
    int rc = check_call(align, n ? 1 : 0, 0, 0, n);
    if (rc) return rc;
    if (n && (!q || !rec || !pstat || !off || !len || !himg || (!dgram && dgram_bytes))) return fcs::set_error(EINVAL, "null pointer");
    if ((uint64_t)q + q_bytes < (uint64_t)q) return fcs::set_error(EINVAL, "q + q_bytes overflows");
    if ((uint64_t)dgram + dgram_bytes < (uint64_t)dgram) return fcs::set_error(EINVAL, "dgram + dgram_bytes overflows");
    if ((uint64_t)q & 7u) return fcs::set_error(EINVAL, "q is not aligned to 8");
    if ((uint64_t)himg & 3u) return fcs::set_error(EINVAL, "himg is not aligned to 4");
    if ((uint64_t)dgram & (align - 1u)) return fcs::set_error(EINVAL, "dgram is not aligned to %u", align);
    int dev = 0, cus = 0;
    if ((rc = fcs::current_device(&dev, &cus))) return rc;
    if (n == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    mux::MParams p{};
    fill_params(p, q, q_bytes, rec, n);
    p.align = align;
    p.pstat = pstat;
    p.off = const_cast<uint64_t *>(off);
    p.len = const_cast<uint32_t *>(len);
    p.himg = (uint32_t *)const_cast<void *>(himg);
    p.dgram = (uint64_t)dgram;
    p.dgram_bytes = dgram_bytes;
    p.mstat = mstat;
    return fcs::launch_with_counter(dev, (void *)st, [&](unsigned long long *ctr) -> int {
        p.ctr = ctr;
        HIPTRY(mux::launch_build(p, cus, st), "launching the mux kernel");
        return 0;
    });
}

int64_t ip_tx_mux_host(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                       const uint64_t *bind, uint32_t S, const struct mux_tcb *tcb, const struct mux_route *rt, uint32_t R,
                       const struct mux_neigh *nb, uint32_t N, uint32_t id0, uint32_t align, void *dgram, uint64_t dgram_bytes,
                       uint32_t *mstat, uint64_t *off, uint32_t *len, struct txf_l2 *l2, void *himg, uint32_t *tnext,
                       uint64_t *counts) {
    t_chunks.clear();
    int rc = check_call(align, S, R, N, n);
    if (rc) return rc;
    if ((rc = check_inputs(q, q_bytes, rec, n, sfirst, bind, S, rt, R, nb, N))) return rc;
    if (!dgram && dgram_bytes) return fcs::set_error(EINVAL, "null pointer");
    if ((rc = check_sfirst(sfirst, S, n))) return rc;
    HostPlan hp;
    hp.mstat.resize(n);
    hp.off.resize(n);
    hp.len.resize(n);
    hp.l2.resize(n);
    hp.himg.resize(n * mux::kImg);
    hp.tnext.resize(S);
    const int64_t planned = mux::plan_batch((const uint8_t *)q, q_bytes, rec, n, sfirst, bind, S, tcb, rt, R, nb, N, id0, align,
                                            hp.mstat.data(), hp.off.data(), hp.len.data(), hp.l2.data(), hp.himg.data(),
                                            hp.tnext.data(), hp.counts);
    uint64_t end = 0;   // rule 8: the last datagram's end (the pad behind it needs no room)
    for (uint64_t k = 0; k < n; k++)
        if (hp.len[k]) end = hp.off[k] + hp.len[k];
    if (end > dgram_bytes)
        return fcs::set_error(ENOSPC, "%lld datagrams need %llu bytes, more than the %llu given", (long long)planned,
                              (unsigned long long)end, (unsigned long long)dgram_bytes);
    int dev = 0, cus = 0;   // no CPU path, also for a batch that plans nothing
    if ((rc = fcs::engine_device0(&dev, &cus))) return rc;
    if (planned) {
        // what travels: the records with a datagram; the others as zero bytes at the end of the one before
        hp.glen.assign(n, 0u);
        hp.goff.assign(n, 0ull);
        uint64_t last = 0;
        for (uint64_t k = 0; k < n; k++) {
            if (hp.mstat[k] & mux::kPlanned) {
                hp.glen[k] = mux::kRecHdr + (hp.len[k] - mux::hl_of(hp.himg[k * mux::kImg + 9]));   // byte 9: the protocol
                hp.goff[k] = rec[k];
                last = rec[k] + hp.glen[k];
            } else {
                hp.goff[k] = last;
            }
        }
        if ((rc = run_host((const uint8_t *)q, rec, n, hp, (uint8_t *)dgram))) return rc;
    }
    for (uint64_t k = 0; k < n; k++) {
        if (mstat) mstat[k] = hp.mstat[k] | ((hp.mstat[k] & mux::kPlanned) ? mux::kBuilt : 0u);
        if (off) off[k] = hp.off[k];
        if (len) len[k] = hp.len[k];
    }
    if (l2 && n) std::memcpy(l2, hp.l2.data(), n * sizeof(txf_l2));
    if (himg && n) std::memcpy(himg, hp.himg.data(), n * mux::kImg);
    if (tnext && S) std::memcpy(tnext, hp.tnext.data(), (size_t)S * 4);
    if (counts) std::memcpy(counts, hp.counts, 32);
    return planned;
}

int fcs_debug_mux_last_launch(char *out, uint64_t cap) {
    return copy_name(mux::last_launch() == mux::Route::kMux ? "mux" : "none", out, cap);
}

int64_t fcs_debug_mux_last_host_chunks(uint64_t *recs, uint64_t cap) {
    return t_chunks.report(recs, cap);
}

}  // extern "C"
