// gro_plan_check.cpp — stand-alone check of the host planning arithmetic of one-pass RX coalescing
// (nstack_amd/csrc/gro_plan.hpp, the header rxr_engine.cpp plans with). Built with
// -fsanitize=address,undefined (tests/c/gro_plan_check.mk) and run by tests/test_gro_model.py: every
// arena here is a heap block of exactly the stated size, so a read past a frame's bytes or past the
// arena's last byte is reported. The plan is compared with a brute-force restatement of rule 3: a
// group is coalescible exactly when its payload ranges cover [lowest seq, highest end) byte by byte
// exactly once and its headers agree. Prints "gro_plan_check: ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <tuple>
#include <vector>

#include "../../nstack_amd/csrc/gro_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

using namespace gro;
using rxr::kHead;
using rxr::kNone32;
using rxr::kNone64;
using rxr::kWhole;

struct Tcp {
    uint32_t hlen = 20, thl = 20, P = 1, seq = 0, sport = 0x8001, tflags = 0x10, ttl = 64, src = 0x0a000001u, win = 0x2000, pad = 0;
};

// A TCP segment in an Ethernet frame: 14 + hlen + thl + P bytes (+ pad zero bytes).
static std::vector<uint8_t> make_frame(const Tcp &t) {
    std::vector<uint8_t> f(14 + t.hlen + t.thl + t.P + t.pad, 0);
    f[12] = 0x08;
    uint8_t *h = f.data() + 14;
    const uint32_t I = t.hlen + t.thl + t.P;
    h[0] = (uint8_t)(0x40 | (t.hlen / 4));
    h[2] = (uint8_t)(I >> 8);
    h[3] = (uint8_t)I;
    h[4] = (uint8_t)(t.seq >> 3);   // any id: it is not compared
    h[8] = (uint8_t)t.ttl;
    h[9] = 6;
    std::memcpy(h + 12, &t.src, 4);
    h[16] = 10;
    h[19] = 2;
    for (uint32_t q = 20; q < t.hlen; q++) h[q] = (uint8_t)q;
    uint8_t *s = h + t.hlen;
    s[0] = (uint8_t)(t.sport >> 8);
    s[1] = (uint8_t)t.sport;
    s[3] = 80;
    s[4] = (uint8_t)(t.seq >> 24);
    s[5] = (uint8_t)(t.seq >> 16);
    s[6] = (uint8_t)(t.seq >> 8);
    s[7] = (uint8_t)t.seq;
    s[12] = (uint8_t)((t.thl / 4) << 4);
    s[13] = (uint8_t)t.tflags;
    s[14] = (uint8_t)(t.win >> 8);
    s[15] = (uint8_t)t.win;
    s[16] = (uint8_t)(t.seq * 7);   // any checksum: it is not looked at
    for (uint32_t q = 20; q < t.thl; q++) s[q] = (uint8_t)(q + 0x40);
    for (uint32_t q = 0; q < t.P; q++) s[t.thl + q] = (uint8_t)(t.seq + q);
    return f;
}

struct Batch {   // frames back to back in a heap block of exactly their size
    uint8_t *p = nullptr;
    uint64_t bytes = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    explicit Batch(const std::vector<std::vector<uint8_t>> &fr) {
        for (const auto &f : fr) bytes += f.size();
        p = (uint8_t *)std::malloc(bytes ? bytes : 1);
        uint64_t at = 0;
        for (const auto &f : fr) {
            if (!f.empty()) std::memcpy(p + at, f.data(), f.size());
            off.push_back(at);
            len.push_back((uint32_t)f.size());
            at += f.size();
        }
    }
    ~Batch() { std::free(p); }
    Batch(const Batch &) = delete;
};

struct Plan {
    std::vector<uint32_t> fstat, dgi, dlen, dlead;
    std::vector<uint64_t> dst, doff;
    int64_t m = 0;
    uint64_t bad = ~0ull;
    void run(const Batch &b, uint32_t align = 1, const uint32_t *verdict = nullptr, uint32_t mask = 0, bool lead = true) {
        const uint64_t n = b.off.size();
        fstat.assign(n, 0xDEADBEEFu);
        dgi.assign(n, 0xDEADBEEFu);
        dlen.assign(n, 0xDEADBEEFu);
        dlead.assign(n, 0xDEADBEEFu);
        dst.assign(n, 0xDEADBEEFull);
        doff.assign(n + 1, 0xDEADBEEFull);
        m = plan_batch(b.p, b.bytes, b.off.data(), b.len.data(), n, 0, verdict, mask, align, fstat.data(), dst.data(), dgi.data(),
                       doff.data(), dlen.data(), lead ? dlead.data() : nullptr, &bad);
    }
};

int main() {
    // ---- rule 2 at its edges, each frame the last bytes of an arena of exactly its size ----
    {
        struct Case {
            Tcp t;
            bool cand;
        };
        std::vector<Case> cs;
        Tcp t;
        cs.push_back({t, true});                      // the smallest candidate: one payload byte
        t.P = 0;
        cs.push_back({t, false});                     // a pure ACK
        t = Tcp();
        t.thl = 60;
        t.hlen = 60;
        cs.push_back({t, true});
        t = Tcp();
        t.P = 32768 - 40;
        cs.push_back({t, true});                      // I == 32768
        t.P++;
        cs.push_back({t, false});                     // I == 32769
        for (uint32_t fl : {0x02u, 0x04u, 0x20u}) {
            t = Tcp();
            t.tflags = 0x10 | fl;
            cs.push_back({t, false});                 // SYN, RST, URG
        }
        t = Tcp();
        t.tflags = 0xd9;
        cs.push_back({t, true});                      // FIN | PSH | ACK | ECE | CWR
        for (const Case &c : cs) {
            Batch b({make_frame(c.t)});
            Plan pl;
            pl.run(b);
            CHECK(pl.m == 1 && pl.fstat[0] == (kWhole | (c.cand ? kCand : 0u)) && pl.dlen[0] == c.t.hlen + c.t.thl + c.t.P);
        }
        // L == 19, thl > L and thl < 20: the TCP header bytes that do not exist are not read
        for (int q = 0; q < 3; q++) {
            t = Tcp();
            std::vector<uint8_t> f = make_frame(t);
            uint8_t *h = f.data() + 14;
            if (q == 0) {
                f.resize(14 + 20 + 19);
                h = f.data() + 14;
                h[3] = 39;
            } else {
                h[20 + 12] = q == 1 ? 0x60 : 0x40;
            }
            Batch b({f});
            Plan pl;
            pl.run(b);
            CHECK(pl.m == 1 && pl.fstat[0] == kWhole);
        }
    }

    // ---- three segments out of order, an unrelated frame between them, no dlead array ----
    {
        Tcp a, b2, c, o;
        a.seq = 1000, a.P = 7, a.tflags = 0x90;
        b2.seq = 1007, b2.P = 3;
        c.seq = 1010, c.P = 5, c.tflags = 0x19, c.pad = 9;
        o.sport = 9, o.seq = 1007, o.P = 2;
        Batch b({make_frame(c), make_frame(o), make_frame(a), make_frame(b2)});
        for (int lead = 0; lead < 2; lead++) {
            Plan pl;
            pl.run(b, 16, nullptr, 0, lead != 0);
            CHECK(pl.m == 2 && pl.dlen[0] == 42 && pl.dlen[1] == 55 && pl.doff[0] == 0 && pl.doff[1] == 48 && pl.doff[2] == 112);
            CHECK(pl.fstat[0] == (kWhole | kCand | kMerged) && pl.fstat[3] == (kWhole | kCand | kMerged) && pl.fstat[1] == (kWhole | kCand));
            CHECK(pl.fstat[2] == (kWhole | kCand | kMerged | kHead | kFin | kPsh));
            CHECK(pl.dgi[1] == 0 && pl.dgi[0] == 1 && pl.dgi[2] == 1 && pl.dgi[3] == 1);
            CHECK(pl.dst[1] == 0 && pl.dst[2] == 48 && pl.dst[3] == 48 + 40 + 7 && pl.dst[0] == 48 + 40 + 10);
            if (lead) CHECK(pl.dlead[0] == 1 && pl.dlead[1] == 2);
        }
        const uint32_t verdict[4] = {0, 0, 0, 1};   // the middle segment dropped: a gap, nothing merges
        Plan pl;
        pl.run(b, 1, verdict, 1);
        CHECK(pl.m == 3 && pl.fstat[3] == rxr::kDropped && !(pl.fstat[0] & kMerged) && !(pl.fstat[2] & kMerged));
    }

    // ---- 32768 members of one byte each, shuffled: the largest group; and one more byte in the next window ----
    {
        std::vector<std::vector<uint8_t>> fr;
        std::vector<uint32_t> perm(32769);
        for (uint32_t q = 0; q < perm.size(); q++) perm[q] = q;
        std::mt19937_64 rng(99);
        for (size_t q = perm.size() - 1; q > 0; q--) std::swap(perm[q], perm[rng() % (q + 1)]);
        const uint32_t base = 0xffff8000u;   // the last window of sequence space, then seq 0
        for (uint32_t q : perm) {
            Tcp t;
            t.seq = base + q;
            fr.push_back(make_frame(t));
        }
        Batch b(fr);
        Plan pl;
        pl.run(b);
        CHECK(pl.m == 2);
        bool ok = true;
        for (size_t i = 0; i < perm.size(); i++) {
            const uint32_t q = perm[i];
            if (q == 32768) ok = ok && pl.fstat[i] == (kWhole | kCand) && pl.dlen[pl.dgi[i]] == 41;
            else ok = ok && pl.fstat[i] == (kWhole | kCand | kMerged | (q ? 0u : kHead)) && pl.dlen[pl.dgi[i]] == 40 + 32768 &&
                      pl.dst[i] == pl.doff[pl.dgi[i]] + (q ? 40 + q : 0);
        }
        CHECK(ok);
    }

    // ---- random batches against the brute-force restatement ----
    {
        std::mt19937_64 rng(2026);
        for (int round = 0; round < 400; round++) {
            const uint32_t n = 2 + rng() % 14;
            const uint32_t base = (round & 1) ? 0xffffffe0u + rng() % 16 : 32768u * (1 + rng() % 3) - 12 + rng() % 8;
            std::vector<Tcp> ts;
            std::vector<std::vector<uint8_t>> fr;
            uint32_t next[2] = {base, base};
            for (uint32_t q = 0; q < n; q++) {
                Tcp t;
                const uint32_t fl = rng() % 2;
                t.sport = 0x8001 + fl;
                t.P = 1 + rng() % 5;
                t.seq = next[fl];
                const uint32_t r = rng() % 16;
                if (r == 0) t.seq += 1;            // a gap
                else if (r == 1) t.seq -= 1;       // an overlap (or a duplicate)
                next[fl] = t.seq + t.P;
                if (rng() % 24 == 0) t.ttl = 63;
                if (rng() % 24 == 0) t.thl = 24;
                if (rng() % 24 == 0) t.tflags |= 0x08;
                if (rng() % 24 == 0) t.tflags |= 0x01;
                if (rng() % 24 == 0) t.tflags |= 0x80;
                if (rng() % 32 == 0) t.tflags |= 0x02;
                if (rng() % 24 == 0) t.win = 0x2001;
                ts.push_back(t);
            }
            for (size_t q = ts.size() - 1; q > 0; q--) std::swap(ts[q], ts[rng() % (q + 1)]);
            for (const Tcp &t : ts) fr.push_back(make_frame(t));
            Batch b(fr);
            Plan pl;
            pl.run(b, 4);
            // brute force
            std::map<std::tuple<uint32_t, uint32_t>, std::vector<uint32_t>> groups;
            std::vector<uint32_t> want(n, kWhole), first_of(n, kNone32);
            std::vector<uint32_t> D(n, 0);
            for (uint32_t i = 0; i < n; i++) {
                D[i] = ts[i].hlen + ts[i].thl + ts[i].P;
                if (ts[i].tflags & 0x26) continue;
                want[i] |= kCand;
                groups[{ts[i].sport, ts[i].seq >> 15}].push_back(i);
            }
            for (auto &kv : groups) {
                const std::vector<uint32_t> &g = kv.second;
                if (g.size() < 2) continue;
                // relative to the window's start: at most 32767 + 5
                std::vector<int> cover(32768 + 8, 0);
                uint32_t lo = ~0u, hi = 0, fi = 0, li = 0;
                for (uint32_t i : g) {
                    const uint32_t r = ts[i].seq & 0x7fff;
                    for (uint32_t q = 0; q < ts[i].P; q++) cover[r + q]++;
                    if (r < lo) lo = r, fi = i;
                    if (r + ts[i].P > hi) hi = r + ts[i].P, li = i;
                }
                bool ok = true;
                for (uint32_t q = lo; q < hi; q++) ok = ok && cover[q] == 1;
                for (uint32_t i : g) {
                    const Tcp &x = ts[i], &f = ts[fi];
                    ok = ok && x.ttl == f.ttl && x.thl == f.thl && x.win == f.win;
                    if (i != li && (x.tflags & 0x09)) ok = false;
                    if (i != fi && (x.tflags & 0x80)) ok = false;
                }
                if (!ok) continue;
                uint32_t sum = 0;
                for (uint32_t i : g) {
                    want[i] |= kMerged;
                    first_of[i] = fi;
                    sum += ts[i].P;
                }
                want[fi] |= kHead | ((ts[li].tflags & 1) ? kFin : 0u) | ((ts[li].tflags & 8) ? kPsh : 0u);
                D[fi] = ts[fi].hlen + ts[fi].thl + sum;
            }
            bool ok = true;
            uint64_t at = 0;
            uint32_t k = 0;
            for (uint32_t i = 0; i < n; i++) {
                ok = ok && pl.fstat[i] == want[i];
                if (first_of[i] != kNone32 && first_of[i] != i) continue;
                ok = ok && k < (uint32_t)pl.m && pl.dlead[k] == i && pl.dlen[k] == D[i] && pl.doff[k] == at && pl.dgi[i] == k && pl.dst[i] == at;
                at += rxr::padded(D[i], 4);
                k++;
            }
            ok = ok && pl.m == (int64_t)k && pl.doff[k] == at;
            for (uint32_t i = 0; i < n && ok; i++) {
                const uint32_t f = first_of[i];
                if (f == kNone32 || f == i) continue;
                ok = pl.dgi[i] == pl.dgi[f] && pl.dst[i] == pl.dst[f] + ts[f].hlen + ts[f].thl + (ts[i].seq - ts[f].seq);
            }
            if (!ok) std::printf("round %d\n", round);
            CHECK(ok);
        }
    }

    // ---- a frame outside the arena: -EINVAL before anything is written ----
    {
        Tcp t;
        Batch b({make_frame(t), make_frame(t)});
        b.off[1] = b.bytes - 10;
        Plan pl;
        pl.run(b);
        CHECK(pl.m == -EINVAL && pl.bad == 1 && pl.fstat[0] == 0xDEADBEEFu && pl.doff[0] == 0xDEADBEEFull);
    }

    if (g_fail) return 1;
    std::printf("gro_plan_check: ok\n");
    return 0;
}
