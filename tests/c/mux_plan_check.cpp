// mux_plan_check.cpp — stand-alone check of the host planning arithmetic of one-pass TX multiplexing
// (nstack_amd/csrc/mux_plan.hpp, the header mux_engine.cpp plans with). Built with
// -fsanitize=address,undefined (tests/c/mux_plan_check.mk) and run by tests/test_mux_model.py: the
// queue, every table and every plan array here is a heap block of exactly the stated size, so a read
// past a record's bytes or a write past an array's end is reported. Covers each rule at its edges,
// duplicate neighbours and S = 0, and runs 400 random batches against a brute-force walk (one record
// at a time, tables searched linearly, the header written byte by byte). Prints "mux_plan_check: ok"
// and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../nstack_amd/csrc/mux_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

using namespace mux;
typedef std::vector<uint8_t> Bytes;

template <class T>
struct Exact {   // a heap block of exactly n elements (one byte for n = 0, never touched)
    T *p;
    uint64_t n;
    explicit Exact(uint64_t n_) : p((T *)std::malloc(n_ ? n_ * sizeof(T) : 1)), n(n_) {
        if (n) std::memset((void *)p, 0xCC, n * sizeof(T));
    }
    ~Exact() { std::free((void *)p); }
    Exact(const Exact &) = delete;
    Exact &operator=(const Exact &) = delete;
    T &operator[](uint64_t i) { return p[i]; }
};

static Bytes record(uint32_t dst, int32_t dport, uint64_t size, uint32_t P) {
    Bytes r(kRecHdr + P);
    const uint32_t src = 0x7f000001u;
    const int32_t sport = 7;
    std::memcpy(&r[0], &src, 4);
    std::memcpy(&r[4], &sport, 4);
    std::memcpy(&r[8], &dst, 4);
    std::memcpy(&r[12], &dport, 4);
    std::memcpy(&r[16], &size, 8);
    for (uint32_t i = 0; i < P; i++) r[kRecHdr + i] = (uint8_t)(i * 7 + dport);
    return r;
}
static Bytes record(uint32_t dst, int32_t dport, uint32_t P) { return record(dst, dport, P, P); }

static mux_route route(uint32_t net, uint32_t mask, uint32_t iface) {
    mux_route r{};
    r.network = net, r.netmask = mask, r.gw = 0xdeadbeefu, r.iface = iface;
    for (int i = 0; i < 6; i++) r.mac[i] = (uint8_t)(iface >> (4 * i));
    return r;
}
static mux_neigh neigh(uint32_t addr, uint8_t tag, uint16_t valid = 1) {
    mux_neigh n{};
    n.addr = addr, n.valid = valid;
    for (int i = 0; i < 6; i++) n.mac[i] = (uint8_t)(tag + i);
    return n;
}

struct Sock {
    uint64_t key;
    mux_tcb tcb;
    std::vector<Bytes> recs;
};

struct Result {
    std::vector<uint32_t> mstat, len, tnext;
    std::vector<uint64_t> off;
    std::vector<uint8_t> l2, himg;
    uint64_t counts[4];
    int64_t planned;
};

// Lays the sockets' records out (each on a multiple of 8, the last ending at the block's end), runs
// plan_batch on exact-size blocks; `mangle` may change rec[] first.
template <class Mangle>
static Result run(const std::vector<Sock> &socks, const std::vector<mux_route> &rt, const std::vector<mux_neigh> &nb, uint32_t id0,
                  uint32_t align, bool with_tcb, Mangle &&mangle) {
    uint64_t n = 0, bytes = 0;
    for (const auto &s : socks)
        for (const auto &r : s.recs) n++, bytes = ((bytes + 7) & ~7ull) + r.size();
    const uint32_t S = (uint32_t)socks.size();
    Exact<uint8_t> q(bytes);
    Exact<uint64_t> rec(n), sfirst(S + 1), bind(S), off(n), counts(4);
    Exact<mux_tcb> tcb(S);
    Exact<mux_route> rtb(rt.size());
    Exact<mux_neigh> nbb(nb.size());
    Exact<uint32_t> mstat(n), len(n), tnext(S);
    Exact<txf_l2> l2(n);
    Exact<uint8_t> himg(n * kImg);
    uint64_t at = 0, k = 0;
    for (uint32_t s = 0; s < S; s++) {
        sfirst[s] = k;
        bind[s] = socks[s].key;
        tcb[s] = socks[s].tcb;
        for (const auto &r : socks[s].recs) {
            at = (at + 7) & ~7ull;
            rec[k++] = at;
            std::memcpy(q.p + at, r.data(), r.size());
            at += r.size();
        }
    }
    sfirst[S] = k;
    for (size_t i = 0; i < rt.size(); i++) rtb[i] = rt[i];
    for (size_t i = 0; i < nb.size(); i++) nbb[i] = nb[i];
    mangle(rec.p, n, bytes);
    CHECK(sfirst_ok(sfirst.p, S, n));
    Result r;
    r.planned = plan_batch(q.p, bytes, rec.p, n, sfirst.p, bind.p, S, with_tcb ? tcb.p : nullptr, rtb.p, (uint32_t)rt.size(), nbb.p,
                           (uint32_t)nb.size(), id0, align, mstat.p, off.p, len.p, l2.p, himg.p, tnext.p, counts.p);
    r.mstat.assign(mstat.p, mstat.p + n);
    r.len.assign(len.p, len.p + n);
    r.off.assign(off.p, off.p + n);
    r.tnext.assign(tnext.p, tnext.p + S);
    r.l2.assign((uint8_t *)l2.p, (uint8_t *)l2.p + n * 12);
    r.himg.assign(himg.p, himg.p + n * kImg);
    std::memcpy(r.counts, counts.p, 32);
    return r;
}
static void keep(uint64_t *, uint64_t, uint64_t) {}

// The brute-force walk: the rules of include/nstack_mux.h for one record at a time, in k order.
static Result brute(const std::vector<Sock> &socks, const std::vector<mux_route> &rt, const std::vector<mux_neigh> &nb, uint32_t id0,
                    uint32_t align, bool with_tcb) {
    Result r{};
    uint64_t at = 0;
    uint32_t id = id0;
    for (const auto &s : socks) {
        const uint32_t proto = (uint32_t)(s.key >> 48);
        const bool valid = proto == 6 || proto == 17;
        uint32_t seq = s.tcb.seq;
        for (const auto &rc : s.recs) {
            uint32_t dst;
            int32_t dport;
            uint64_t P;
            std::memcpy(&dst, &rc[8], 4), std::memcpy(&dport, &rc[12], 4), std::memcpy(&P, &rc[16], 8);
            uint32_t st = 0;
            int ri = -1, ni = -1;
            if (!valid || P != rc.size() - kRecHdr || dport < 0 || dport > 65535) st = kBadRec;   // (a size that lies is outside q only for the last record: not generated)
            if (!st) {
                if (proto == 17 ? (P == 0 || P >= 65507) : P > 65495) st |= kBadSize;
                if (proto == 6 && !with_tcb) st |= kNoTcb;
            }
            if (!st) {
                for (size_t i = 0; i < rt.size() && ri < 0; i++)
                    if (rt[i].network == dst) ri = (int)i;
                for (size_t i = 0; i < rt.size() && ri < 0; i++)
                    if (rt[i].network == (dst & rt[i].netmask)) ri = (int)i;
                for (size_t i = 0; i < rt.size() && ri < 0; i++)
                    if (rt[i].network == 0) ri = (int)i;
                if (ri < 0) st = kNoRoute;
            }
            if (!st) {
                for (size_t i = 0; i < nb.size() && ni < 0; i++)
                    if (nb[i].valid && nb[i].addr == dst) ni = (int)i;
                if (ni < 0) st = kNoNeigh;
            }
            uint8_t img[kImg] = {0}, l2[12] = {0};
            uint32_t len = 0;
            r.off.push_back(at);
            if (!st) {
                st = kPlanned;
                const uint32_t hl = proto == 17 ? 28 : 40, L = hl + (uint32_t)P, src = rt[ri].iface;
                const uint32_t sport = (uint32_t)(s.key >> 32) & 0xffff;
                const uint8_t ip[20] = {0x45, 0, (uint8_t)(L >> 8), (uint8_t)L, (uint8_t)(id >> 8), (uint8_t)id, 0x40, 0, 64, (uint8_t)proto, 0, 0,
                                        (uint8_t)(src >> 24), (uint8_t)(src >> 16), (uint8_t)(src >> 8), (uint8_t)src,
                                        (uint8_t)(dst >> 24), (uint8_t)(dst >> 16), (uint8_t)(dst >> 8), (uint8_t)dst};
                std::memcpy(img, ip, 20);
                uint32_t sum = 0;
                for (int i = 0; i < 20; i += 2) sum += ((uint32_t)img[i] << 8) | img[i + 1];
                while (sum >> 16) sum = (sum & 0xffff) + (sum >> 16);
                sum = ~sum & 0xffff;
                img[10] = (uint8_t)(sum >> 8), img[11] = (uint8_t)sum;
                img[20] = (uint8_t)(sport >> 8), img[21] = (uint8_t)sport, img[22] = (uint8_t)(dport >> 8), img[23] = (uint8_t)dport;
                if (proto == 17) {
                    img[24] = (uint8_t)((8 + P) >> 8), img[25] = (uint8_t)(8 + P);
                } else {
                    for (int b = 0; b < 4; b++) img[24 + b] = (uint8_t)(seq >> (24 - 8 * b)), img[28 + b] = (uint8_t)(s.tcb.ack >> (24 - 8 * b));
                    img[32] = 0x50, img[33] = s.tcb.flags, img[34] = (uint8_t)(s.tcb.win >> 8), img[35] = (uint8_t)s.tcb.win;
                    seq += (uint32_t)P;
                }
                id = (id + 1) & 0xffff;
                len = L;
                at += (L + align - 1) / align * align;
                std::memcpy(l2, nb[ni].mac, 6), std::memcpy(l2 + 6, rt[ri].mac, 6);
                r.planned++;
            }
            r.counts[2] += st == kNoRoute, r.counts[3] += st == kNoNeigh;
            r.mstat.push_back(st);
            r.len.push_back(len);
            r.l2.insert(r.l2.end(), l2, l2 + 12);
            r.himg.insert(r.himg.end(), img, img + kImg);
        }
        r.tnext.push_back(valid && proto == 6 && with_tcb ? seq : 0u);
    }
    r.counts[0] = (uint64_t)r.planned, r.counts[1] = at;
    return r;
}

static bool same(const Result &a, const Result &b) {
    return a.planned == b.planned && a.mstat == b.mstat && a.len == b.len && a.off == b.off && a.tnext == b.tnext && a.l2 == b.l2 &&
           a.himg == b.himg && std::memcmp(a.counts, b.counts, 32) == 0;
}

static const uint32_t NET = 0x0a000000u, IF1 = 0x0a000001u, H = 0x0a000002u;
static uint64_t key(uint32_t proto, uint32_t port) { return ((uint64_t)proto << 48) | ((uint64_t)port << 32) | IF1; }

int main() {
    const std::vector<mux_route> rt1 = {route(NET, 0xffffff00u, IF1)};
    const std::vector<mux_neigh> nb1 = {neigh(H, 1)};
    const mux_tcb t0{0xffffff00u, 5, 502, 0x18, 0};

    // rule 1 at its edges
    {
        std::vector<Sock> s = {{key(17, 9), t0, {record(H, 53, 4), record(H, 0, 1), record(H, 65535, 1), record(H, 65536, 1), record(H, -1, 1),
                                                 record(H, 53, 1ull << 63, 0), record(H, 53, 4)}}};
        Result r = run(s, rt1, nb1, 0, 4, true, keep);
        CHECK((r.mstat == std::vector<uint32_t>{kPlanned, kPlanned, kPlanned, kBadRec, kBadRec, kBadRec, kPlanned}));
        CHECK(same(r, brute(s, rt1, nb1, 0, 4, true)));
        // the last record ends exactly at q_bytes: planned; one byte more claimed: outside
        std::vector<Sock> s2 = {{key(17, 9), t0, {record(H, 53, 4), record(H, 53, 5, 4)}}};
        r = run(s2, rt1, nb1, 0, 4, true, keep);
        CHECK((r.mstat == std::vector<uint32_t>{kPlanned, kBadRec}));
        // a start that is no multiple of 8; a header that crosses the end; a start behind the end
        r = run(s, rt1, nb1, 0, 4, true, [](uint64_t *rec, uint64_t, uint64_t bytes) {
            rec[0] += 4;
            rec[1] = (bytes - 23 + 7) & ~7ull;
            rec[2] = bytes + 8;
            rec[6] = ~0ull & ~7ull;
        });
        CHECK(r.mstat[0] == kBadRec && r.mstat[1] == kBadRec && r.mstat[2] == kBadRec && r.mstat[6] == kBadRec && r.planned == 0);
        // an invalid key
        std::vector<Sock> s3 = {{key(1, 9), t0, {record(H, 53, 4)}}, {key(17, 9) | (1ull << 56), t0, {record(H, 53, 4)}}, {0, t0, {record(H, 53, 4)}}};
        r = run(s3, rt1, nb1, 0, 4, true, keep);
        CHECK((r.mstat == std::vector<uint32_t>{kBadRec, kBadRec, kBadRec}) && r.tnext == std::vector<uint32_t>(3, 0u));
    }
    // rule 2 at its edges, and the seq wrap across unplanned records
    {
        std::vector<Sock> s = {{key(17, 9), t0, {record(H, 53, 0), record(H, 53, 1), record(H, 53, 65506), record(H, 53, 65507)}},
                               {key(6, 9), t0, {record(H, 80, 0), record(H, 80, 0x100), record(H, 80, 65496), record(H, 80, 65495), record(H, 80, 1)}}};
        Result r = run(s, rt1, nb1, 0xfffe, 16, true, keep);
        CHECK((r.mstat == std::vector<uint32_t>{kBadSize, kPlanned, kPlanned, kBadSize, kPlanned, kPlanned, kBadSize, kPlanned, kPlanned}));
        CHECK(same(r, brute(s, rt1, nb1, 0xfffe, 16, true)));
        CHECK(r.tnext[1] == 0xffffff00u + 0x100u + 65495u + 1u && r.tnext[0] == 0);
        CHECK(r.himg[1 * kImg + 4] == 0xff && r.himg[1 * kImg + 5] == 0xfe && r.himg[4 * kImg + 4] == 0 && r.himg[4 * kImg + 5] == 0);   // the id wraps
        CHECK(r.himg[7 * kImg + 24] == 0 && r.himg[7 * kImg + 27] == 0);                                                                      // the seq wrapped
        r = run(s, rt1, nb1, 0, 16, false, keep);
        CHECK(r.mstat[4] == kNoTcb && r.mstat[6] == (kNoTcb | kBadSize) && r.mstat[1] == kPlanned && r.tnext[1] == 0);
        CHECK(same(r, brute(s, rt1, nb1, 0, 16, false)));
    }
    // rule 3: the three steps
    {
        const uint32_t x = NET + 9;
        const std::vector<mux_neigh> nb = {neigh(x, 1), neigh(NET + 3, 2), neigh(0x08080808u, 3), neigh(0, 4)};
        std::vector<Sock> s = {{key(17, 9), t0, {record(x, 1, 1), record(NET + 3, 1, 1), record(0x08080808u, 1, 1), record(0, 1, 1)}}};
        const std::vector<mux_route> exact_behind = {route(NET, 0xffffff00u, 1), route(x, 0xffffffffu, 2)};
        Result r = run(s, exact_behind, nb, 0, 4, true, keep);
        CHECK(r.himg[15] == 2 && r.himg[kImg + 15] == 1 && r.mstat[2] == kNoRoute && r.mstat[3] == kNoRoute && r.counts[2] == 2);
        const std::vector<mux_route> two_masks = {route(NET, 0xffff0000u, 1), route(NET, 0xffffff00u, 2), route(0, 0xff000000u, 3)};
        r = run(s, two_masks, nb, 0, 4, true, keep);
        CHECK(r.himg[15] == 1 && r.himg[kImg + 15] == 1 && r.himg[2 * kImg + 15] == 3 && r.himg[3 * kImg + 15] == 3);   // step 3, and step 1 on dst 0
        const std::vector<mux_route> dflt2 = {route(0, 0, 7)};
        r = run(s, dflt2, nb, 0, 4, true, keep);
        CHECK(r.planned == 4 && r.himg[15] == 7);                                                                        // the default through step 2
        r = run(s, {}, nb, 0, 4, true, keep);
        CHECK(r.planned == 0 && r.counts[2] == 4);
        CHECK(same(r, brute(s, {}, nb, 0, 4, true)));
    }
    // rule 4: duplicate, invalid and missing neighbours
    {
        const std::vector<mux_neigh> nb = {neigh(H + 1, 9, 0), neigh(H, 1), neigh(H, 2), neigh(H + 1, 3), neigh(H + 2, 4, 0)};
        std::vector<Sock> s = {{key(17, 9), t0, {record(H, 1, 1), record(H + 1, 1, 1), record(H + 2, 1, 1), record(H + 3, 1, 1)}}};
        Result r = run(s, rt1, nb, 0, 8, true, keep);
        CHECK((r.mstat == std::vector<uint32_t>{kPlanned, kPlanned, kNoNeigh, kNoNeigh}) && r.l2[0] == 1 && r.l2[12] == 3 && r.counts[3] == 2);
        CHECK(r.l2[24] == 0 && r.len[2] == 0 && r.off[2] == 64 && r.off[3] == 64);
        CHECK(same(r, brute(s, rt1, nb, 0, 8, true)));
        r = run(s, rt1, {}, 0, 8, true, keep);
        CHECK(r.planned == 0 && r.counts[3] == 4);
    }
    // S = 0, and sockets without records
    {
        Result r = run({}, rt1, nb1, 0, 4, true, keep);
        CHECK(r.planned == 0 && r.counts[1] == 0);
        std::vector<Sock> s = {{key(6, 1), t0, {}}, {key(17, 2), t0, {record(H, 1, 3)}}, {key(6, 3), t0, {}}};
        r = run(s, rt1, nb1, 0, 4, true, keep);
        CHECK(r.planned == 1 && r.tnext[0] == t0.seq && r.tnext[1] == 0 && r.tnext[2] == t0.seq);
        uint64_t bad[3] = {0, 2, 1};
        CHECK(!sfirst_ok(bad, 2, 1) && !sfirst_ok(bad + 1, 1, 1) && sfirst_ok(bad, 1, 2) && sfirst_ok(nullptr, 0, 0) && !sfirst_ok(nullptr, 0, 1));
        CHECK(check_geometry(4, 65536, 256, 65536) == 0 && check_geometry(2, 0, 0, 0) && check_geometry(256, 0, 0, 0) &&
              check_geometry(12, 0, 0, 0) && check_geometry(4, 65537, 0, 0) && check_geometry(4, 0, 257, 0) && check_geometry(4, 0, 0, 65537));
    }
    // random batches against the brute-force walk
    std::mt19937 rng(12345);
    for (int it = 0; it < 400; it++) {
        const uint32_t S = rng() % 6, R = rng() % 5, N = rng() % 12;
        const uint32_t aligns[] = {4, 8, 16, 32, 64, 128};
        std::vector<mux_route> rt;
        for (uint32_t i = 0; i < R; i++) {
            const uint32_t kind = rng() % 4;
            rt.push_back(kind == 0 ? route(NET + (rng() % 8), 0xffffffffu, 100 + i) : kind == 1 ? route(NET, 0xfffffff8u, 100 + i)
                         : kind == 2 ? route(NET, 0xffffff00u, 100 + i) : route(0, (rng() & 1) ? 0 : 0xff000000u, 100 + i));
        }
        std::vector<mux_neigh> nb;
        for (uint32_t i = 0; i < N; i++) nb.push_back(neigh(NET + (rng() % 10), (uint8_t)(10 * i), (uint16_t)(rng() % 4 != 0)));
        std::vector<Sock> socks;
        for (uint32_t s = 0; s < S; s++) {
            Sock so{key((rng() % 8 == 0) ? 1 : (rng() & 1) ? 6 : 17, 1000 + s), mux_tcb{(uint32_t)rng() | 0xfffff000u, (uint32_t)rng(), (uint16_t)rng(), (uint8_t)rng(), 0}, {}};
            const uint32_t cnt = rng() % 6;
            for (uint32_t i = 0; i < cnt; i++) {
                const uint32_t P = rng() % 16 == 0 ? 0 : rng() % 600;
                const int32_t dport = rng() % 12 == 0 ? (int32_t)(65536 + rng() % 5) - (int32_t)(rng() % 2) * 70000 : (int32_t)(rng() % 65536);
                so.recs.push_back(record(rng() % 9 == 0 ? 0x08080808u : NET + (rng() % 10), dport, P));
            }
            socks.push_back(so);
        }
        const uint32_t align = aligns[rng() % 6], id0 = rng() & 0x1ffff;
        const bool with_tcb = rng() % 5 != 0;
        CHECK(same(run(socks, rt, nb, id0, align, with_tcb, keep), brute(socks, rt, nb, id0, align, with_tcb)));
        if (g_fail) break;
    }
    if (g_fail) return 1;
    std::printf("mux_plan_check: ok\n");
    return 0;
}
