// rxr_plan_check.cpp — stand-alone check of the host planning arithmetic of one-pass RX reassembly
// (nstack_amd/csrc/rxr_plan.hpp, the header rxr_engine.cpp plans with). Built with
// -fsanitize=address,undefined (tests/c/rxr_plan_check.mk) and run by tests/test_rxr_model.py: every
// arena here is a heap block of exactly the stated size, so a read past a frame's bytes or past the
// arena's last byte is reported. Prints "rxr_plan_check: ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../nstack_amd/csrc/rxr_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

using namespace rxr;

// An IPv4 frame: 14 + hlen + L bytes (+ pad zero bytes), foff in host order.
static std::vector<uint8_t> make_frame(uint32_t hlen, uint32_t L, uint32_t foff, uint32_t id, uint32_t src = 0x0a000001u,
                                       uint32_t pad = 0, uint8_t proto = 17) {
    std::vector<uint8_t> f(14 + hlen + L + pad, 0);
    f[12] = 0x08;
    uint8_t *h = f.data() + 14;
    const uint32_t I = hlen + L;
    h[0] = (uint8_t)(0x40 | (hlen / 4));
    h[2] = (uint8_t)(I >> 8);
    h[3] = (uint8_t)I;
    h[4] = (uint8_t)(id >> 8);
    h[5] = (uint8_t)id;
    h[6] = (uint8_t)(foff >> 8);
    h[7] = (uint8_t)foff;
    h[8] = 64;
    h[9] = proto;
    std::memcpy(h + 12, &src, 4);
    h[16] = 10;
    h[19] = 2;
    for (uint32_t q = 0; q < L; q++) h[hlen + q] = (uint8_t)(q * 7 + id);
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
    void run(const Batch &b, uint32_t flags = 0, uint32_t align = 1, const uint32_t *verdict = nullptr, uint32_t mask = 0) {
        const uint64_t n = b.off.size();
        fstat.assign(n, 0xDEADBEEFu);
        dgi.assign(n, 0xDEADBEEFu);
        dlen.assign(n, 0xDEADBEEFu);
        dlead.assign(n, 0xDEADBEEFu);
        dst.assign(n, 0xDEADBEEFull);
        doff.assign(n + 1, 0xDEADBEEFull);
        m = plan_batch(b.p, b.bytes, b.off.data(), b.len.data(), n, flags, verdict, mask, align, fstat.data(), dst.data(),
                       dgi.data(), doff.data(), dlen.data(), dlead.data(), &bad);
    }
};

int main() {
    // ---- the arithmetic ----
    CHECK(check_geometry(0, 1) == 0 && check_geometry(1, 128) == 0 && check_geometry(2, 1) == -EINVAL);
    CHECK(check_geometry(0, 0) == -EINVAL && check_geometry(0, 3) == -EINVAL && check_geometry(0, 256) == -EINVAL);
    CHECK(padded(0, 1) == 0 && padded(1, 16) == 16 && padded(65535, 128) == 65536 && padded(48, 16) == 48);
    CHECK(has_room(0, 0, 0) && has_room(10, 5, 15) && !has_room(10, 5, 14) && !has_room(16, 0, 15) &&
          !has_room(~0ull, 1, ~0ull));

    // ---- frames of 0..40 bytes, each the last bytes of an arena of exactly that size; with the
    //      trailer flag too: nothing behind the frame is read ----
    for (uint32_t flags = 0; flags < 2; flags++) {
        for (uint32_t F = 0; F <= 40; F++) {
            std::vector<uint8_t> f = make_frame(20, 20, 0, 1);   // 54 bytes, cut to F: ip_len then exceeds P
            f.resize(F);
            Batch b({f});
            Plan pl;
            pl.run(b, flags);
            const uint32_t T = flags ? 4 : 0;
            const uint32_t want = F < 14 + T ? kNotIpv4 : (F - 14 - T < 20 ? kBadHdr : kBadLen);
            CHECK(pl.m == 0 && pl.fstat[0] == want && pl.doff[0] == 0 && pl.dst[0] == kNone64 && pl.dgi[0] == kNone32);
        }
    }
    {   // the shortest whole datagram ends at the arena's last byte
        Batch b({make_frame(20, 0, 0, 1)});
        Plan pl;
        pl.run(b);
        CHECK(pl.m == 1 && pl.fstat[0] == kWhole && pl.dlen[0] == 20 && pl.doff[1] == 20 && pl.dst[0] == 0 && pl.dlead[0] == 0);
    }

    // ---- frames outside the arena, offsets near 2^64: -EINVAL before anything is written ----
    {
        Batch b({make_frame(20, 8, 0, 1), make_frame(20, 8, 0, 2)});
        const uint64_t offs[4] = {b.bytes - 41, ~0ull, ~0ull - 20, b.bytes + 1};
        for (uint64_t o : offs) {
            b.off[1] = o;
            Plan pl;
            pl.run(b);
            CHECK(pl.m == -EINVAL && pl.bad == 1 && pl.fstat[0] == 0xDEADBEEFu && pl.doff[0] == 0xDEADBEEFull);
        }
        b.off[1] = b.bytes;   // an empty frame at the arena's end is inside it
        b.len[1] = 0;
        Plan pl;
        pl.run(b);
        CHECK(pl.m == 1 && pl.fstat[1] == kNotIpv4);
    }

    // ---- one group of 8185 fragments of 8 bytes behind a 60-byte head header, then shuffled ----
    {
        const uint32_t cnt = 8185, total = 8 * 8184 + 3;
        std::vector<std::vector<uint8_t>> fr;
        for (uint32_t q = 0; q < cnt; q++) fr.push_back(make_frame(q ? 20 : 60, q + 1 < cnt ? 8 : 3, (q + 1 < cnt ? 0x2000u : 0u) | q, 77, 5, 30));
        std::vector<uint32_t> perm(cnt);
        for (uint32_t q = 0; q < cnt; q++) perm[q] = q;
        for (int pass = 0; pass < 2; pass++) {
            std::vector<std::vector<uint8_t>> in;
            for (uint32_t q = 0; q < cnt; q++) in.push_back(fr[perm[q]]);
            Batch b(in);
            Plan pl;
            pl.run(b, 0, 16);
            CHECK(pl.m == 1 && pl.dlen[0] == 60 + total && pl.doff[0] == 0 && pl.doff[1] == padded(60 + total, 16));
            bool ok = true;
            for (uint32_t q = 0; q < cnt; q++) {
                const uint32_t j = perm[q];
                ok = ok && pl.dgi[q] == 0 && pl.dst[q] == (j ? 60 + 8ull * j : 0ull) && pl.fstat[q] == (kFrag | (j ? 0u : kHead));
                if (j == 0) ok = ok && pl.dlead[0] == q;
            }
            CHECK(ok);
            std::mt19937_64 rng(12345);
            for (uint32_t q = cnt - 1; q > 0; q--) std::swap(perm[q], perm[rng() % (q + 1)]);
        }
        // without its 4000th fragment, or with it twice: every fragment incomplete, nothing delivered
        for (int twice = 0; twice < 2; twice++) {
            std::vector<std::vector<uint8_t>> in(fr);
            if (twice) in.push_back(fr[4000]);
            else in.erase(in.begin() + 4000);
            Batch b(in);
            Plan pl;
            pl.run(b);
            bool ok = pl.m == 0 && pl.doff[0] == 0;
            for (size_t q = 0; q < in.size(); q++) ok = ok && (pl.fstat[q] & kIncomplete) && pl.dst[q] == kNone64;
            CHECK(ok);
        }
    }

    // ---- 10^5 two-fragment groups and every 10th a whole datagram between them, fully shuffled:
    //      the same datagrams in head order; capacity exact and one short ----
    {
        const uint32_t G = 100000;
        std::vector<std::vector<uint8_t>> fr;
        std::vector<uint32_t> gid;   // the group of frame q, G + q for a whole one
        for (uint32_t g = 0; g < G; g++) {
            const uint32_t id = g & 0xffff, src = 0x0a000000u + (g >> 16), L1 = 1 + g % 13;
            fr.push_back(make_frame(20 + 4 * (g % 3), 16, 0x2000u, id, src));
            gid.push_back(g);
            fr.push_back(make_frame(20, L1, 2, id, src, 18));
            gid.push_back(g);
            if (g % 10 == 0) {
                fr.push_back(make_frame(24, g % 50, 0, id, src, 0, 6));   // another protocol: its own key, and whole anyway
                gid.push_back(G + g);
            }
        }
        std::vector<uint32_t> perm(fr.size());
        for (uint32_t q = 0; q < perm.size(); q++) perm[q] = q;
        std::mt19937_64 rng(777);
        for (size_t q = perm.size() - 1; q > 0; q--) std::swap(perm[q], perm[rng() % (q + 1)]);
        std::vector<std::vector<uint8_t>> in;
        for (uint32_t q : perm) in.push_back(fr[q]);
        Batch b(in);
        Plan pl;
        pl.run(b, 0, 8);
        CHECK(pl.m == (int64_t)(G + G / 10));
        bool ok = true;
        uint64_t at = 0;
        for (int64_t k = 0; k < pl.m && ok; k++) {
            const uint32_t lead = pl.dlead[k], src_frame = perm[lead];
            ok = ok && (k == 0 || pl.dlead[k - 1] < lead) && pl.doff[k] == at && pl.dgi[lead] == (uint32_t)k && pl.dst[lead] == at;
            const uint32_t g = gid[src_frame];
            const uint32_t want = g >= G ? 24 + (g - G) % 50 : 20 + 4 * (g % 3) + 16 + 1 + g % 13;
            ok = ok && pl.dlen[k] == want;
            at += padded(want, 8);
        }
        CHECK(ok && pl.doff[pl.m] == at);
        ok = true;
        for (size_t q = 0; q < in.size() && ok; q++) {   // every second fragment sits behind its own head
            const uint32_t g = gid[perm[q]];
            if (g < G && !(pl.fstat[q] & kHead)) {
                const uint32_t k = pl.dgi[q];
                ok = k < (uint32_t)pl.m && gid[perm[pl.dlead[k]]] == g && pl.dst[q] == pl.doff[k] + 20 + 4 * (g % 3) + 16;
            }
        }
        CHECK(ok);
        const uint64_t need = pl.doff[pl.m - 1] + pl.dlen[pl.m - 1];   // the last datagram's end: the capacity that is exact
        bool all = true;
        for (int64_t k = 0; k < pl.m; k++) all = all && has_room(pl.doff[k], pl.dlen[k], need);
        CHECK(all && !has_room(pl.doff[pl.m - 1], pl.dlen[pl.m - 1], need - 1) && has_room(pl.doff[pl.m - 2], pl.dlen[pl.m - 2], need - 1));
    }

    // ---- rule 1, the trailer, and a too-big group ----
    {
        std::vector<std::vector<uint8_t>> fr = {make_frame(20, 30, 0, 1, 1, 4), make_frame(20, 30, 0, 2, 1, 4),
                                                make_frame(60, 65472, 0x2000u, 3, 1, 4), make_frame(20, 43, 65472 >> 3, 3, 1, 4)};
        const uint32_t verdict[4] = {0x40, 0x01, 0, 0};
        Batch b(fr);
        Plan pl;
        pl.run(b, kFlagTrailer, 1, verdict, 0x3b);
        CHECK(pl.m == 1 && pl.fstat[0] == kWhole && pl.fstat[1] == kDropped && pl.fstat[2] == (kFrag | kHead | kTooBig) &&
              pl.fstat[3] == (kFrag | kTooBig) && pl.dlen[0] == 50);
        pl.run(b, 0);   // without the flag the four bytes are padding: the same datagrams, and nothing is dropped
        CHECK(pl.m == 2 && pl.dlen[0] == 50 && pl.dlen[1] == 50);
    }

    if (g_fail) return 1;
    std::printf("rxr_plan_check: ok\n");
    return 0;
}
