// dmx_plan_check.cpp — stand-alone check of the host planning arithmetic of one-pass RX demultiplexing
// (nstack_amd/csrc/dmx_plan.hpp, the header dmx_engine.cpp plans with). Built with
// -fsanitize=address,undefined (tests/c/dmx_plan_check.mk) and run by tests/test_dmx_model.py: every
// arena and every plan array here is a heap block of exactly the stated size, so a read past a
// datagram's bytes or a write past an array's end is reported. Covers each rule at its edges, duplicate
// keys and S = 0, and runs 400 random batches against a brute-force restatement (for each socket, walk
// k upward and append). Prints "dmx_plan_check: ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "../../nstack_amd/csrc/dmx_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

using namespace dmx;
typedef std::vector<uint8_t> Bytes;

static const uint32_t A = 0x0a000002u, B = 0xc0a80101u;

static Bytes ip(uint8_t proto, const Bytes &seg, uint32_t dst = A, uint32_t hlen = 20, uint32_t src = 0x0a000001u) {
    Bytes d(hlen + seg.size(), 1);
    const uint32_t I = (uint32_t)d.size();
    d[0] = (uint8_t)(0x40 | (hlen / 4));
    d[2] = (uint8_t)(I >> 8);
    d[3] = (uint8_t)I;
    d[9] = proto;
    for (int b = 0; b < 4; b++) {
        d[12 + b] = (uint8_t)(src >> (24 - 8 * b));
        d[16 + b] = (uint8_t)(dst >> (24 - 8 * b));
    }
    if (!seg.empty()) std::memcpy(d.data() + hlen, seg.data(), seg.size());
    return d;
}
static Bytes udp(uint32_t P, uint32_t dport, uint32_t dst = A, uint32_t hlen = 20, uint32_t sport = 0x1234) {
    Bytes s(8 + P);
    s[0] = (uint8_t)(sport >> 8), s[1] = (uint8_t)sport, s[2] = (uint8_t)(dport >> 8), s[3] = (uint8_t)dport;
    for (uint32_t q = 0; q < P; q++) s[8 + q] = (uint8_t)(q * 5 + dport);
    return ip(17, s, dst, hlen);
}
static Bytes tcp(uint32_t P, uint32_t dport, uint32_t dst = A, uint32_t thl = 20, uint8_t fl = 0x18, uint32_t hlen = 20) {
    Bytes s(thl + P, 2);
    s[0] = 0x80, s[1] = 1, s[2] = (uint8_t)(dport >> 8), s[3] = (uint8_t)dport;
    s[12] = (uint8_t)((thl / 4) << 4);
    s[13] = fl;
    for (uint32_t q = 0; q < P; q++) s[thl + q] = (uint8_t)(q * 3 + dport);
    return ip(6, s, dst, hlen);
}

struct Batch {   // datagrams back to back in a heap block of exactly their size
    uint8_t *p = nullptr;
    uint64_t bytes = 0;
    std::vector<uint64_t> off;
    std::vector<uint32_t> len;
    explicit Batch(const std::vector<Bytes> &dg) {
        for (const auto &d : dg) bytes += d.size();
        p = (uint8_t *)std::malloc(bytes ? bytes : 1);
        uint64_t at = 0;
        for (const auto &d : dg) {
            if (!d.empty()) std::memcpy(p + at, d.data(), d.size());
            off.push_back(at);
            len.push_back((uint32_t)d.size());
            at += d.size();
        }
    }
    ~Batch() { std::free(p); }
    Batch(const Batch &) = delete;
};

template <class T>
struct Exact {   // a heap block of exactly k elements (vectors may hold capacity beyond their size)
    T *p;
    uint64_t k;
    explicit Exact(uint64_t k_, T fill) : p((T *)std::malloc(k_ ? k_ * sizeof(T) : 1)), k(k_) {
        for (uint64_t i = 0; i < k; i++) p[i] = fill;
    }
    ~Exact() { std::free(p); }
    Exact(const Exact &) = delete;
    T &operator[](uint64_t i) { return p[i]; }
};

struct Plan {
    Exact<uint32_t> dstat, dsock, scnt;
    Exact<uint64_t> rec, sbase;
    uint64_t bad = ~0ull, counters[4] = {9, 9, 9, 9};
    int64_t r = 0;
    Plan(uint64_t n, uint32_t S) : dstat(n, 0xDEADBEEFu), dsock(n, 0xDEADBEEFu), scnt(S, 0xDEADBEEFu), rec(n, 0xDEADBEEFull), sbase((uint64_t)S + 1, 0xDEADBEEFull) {}
    void run(const Batch &b, const std::vector<uint64_t> &bind, uint32_t align = 8, const uint32_t *verdict = nullptr,
             uint32_t mask = 0, uint64_t out_bytes = ~0ull) {
        Exact<uint64_t> keys(bind.size(), 0);
        for (size_t s = 0; s < bind.size(); s++) keys[s] = bind[s];
        r = plan_batch(b.p, out_bytes == ~0ull ? b.bytes : out_bytes, b.off.data(), b.len.data(), verdict, b.off.size(), keys.p,
                       (uint32_t)bind.size(), mask, align, dstat.p, dsock.p, rec.p, sbase.p, scnt.p, &bad, counters);
    }
};

static void rules() {
    const std::vector<uint64_t> bind = {key_of(17, 53, A), key_of(6, 80, A)};
    {   // rule 1: D < 20, hlen below 20 and beyond D; the verdict mask and RXD_NO_ROOM; outside out_bytes
        Bytes tiny = udp(4, 53);
        tiny.resize(19);
        Bytes h16 = udp(4, 53), h60 = udp(4, 53), exact = ip(17, Bytes(), A, 20);
        h16[0] = 0x44;
        h60[0] = 0x4f;
        Batch b({tiny, h16, h60, exact, udp(4, 53), udp(4, 53), udp(4, 53), udp(4, 53)});
        const uint32_t verdict[8] = {0, 0, 0, 0, 0x100, kDgNoRoom, 0x200, 0};
        Plan p(8, 2);
        p.run(b, bind, 8, verdict, 0x100, b.bytes - 1);
        CHECK(p.r == 1 && p.counters[0] == 1 && p.counters[3] == 6 && p.counters[2] == 0);
        CHECK(p.dstat[0] == kDropped && p.dstat[1] == kDropped && p.dstat[2] == kDropped);
        CHECK(p.dstat[3] == kShort);                                   // hlen == D passes rule 1; L = 0 < 8
        CHECK(p.dstat[4] == kDropped && p.dstat[5] == kDropped && p.dstat[6] == kQueued && p.dstat[7] == kDropped);
        CHECK(p.rec[6] == 0 && p.sbase[0] == 0 && p.sbase[1] == 32 && p.sbase[2] == 32 && p.scnt[0] == 1 && p.scnt[1] == 0);
        CHECK(p.rec[7] == kNone64 && p.dsock[7] == kNone32 && p.dsock[6] == 0);
    }
    {   // rules 2-4 at their edges
        Bytes thl16 = tcp(5, 80), thl_long = tcp(5, 80);
        thl16[32] = 0x40;
        thl_long[32] = 0x70;   // 28 > L = 25
        Batch b({ip(1, Bytes(12, 3)), ip(17, Bytes(7, 0)), udp(0, 53), ip(6, Bytes(19, 0)), thl16, thl_long, tcp(0, 80),
                 tcp(1, 80), tcp(3, 80, A, 60), tcp(3, 80, A, 20, 0x02), tcp(3, 80, A, 20, 0x14), tcp(1, 80, A, 20, 0x01),
                 udp(3, 53, A, 60)});
        Plan p(13, 2);
        p.run(b, bind, 16);
        const uint32_t want[13] = {kNoProto, kShort, kQueued, kShort, kShort, kShort, kCtrl, kQueued, kQueued, kCtrl, kCtrl, kQueued, kQueued};
        for (int k = 0; k < 13; k++) CHECK(p.dstat[k] == want[k]);
        CHECK(p.dsock[6] == 1 && p.dsock[9] == 1 && p.dsock[10] == 1 && p.dsock[0] == kNone32 && p.dsock[1] == kNone32);
        CHECK(p.r == 5 && p.scnt[0] == 2 && p.scnt[1] == 3);
        CHECK(p.rec[2] == 0 && p.rec[12] == 32 && p.sbase[1] == 64 && p.rec[7] == 64 && p.rec[8] == 96 && p.rec[11] == 128 && p.sbase[2] == 160);
    }
    {   // rule 5: exact match only; duplicate keys belong to the lowest index; S = 0
        const uint64_t k0 = key_of(17, 53, A), k1 = key_of(6, 80, B);
        Batch b({udp(1, 53), tcp(1, 80, B), udp(1, 54), udp(1, 53, B), tcp(1, 53), tcp(0, 81, A, 20, 0x12), udp(2, 53)});
        Plan p(7, 5);
        p.run(b, {k1, k0, k0, k1, k0}, 8);
        CHECK(p.dsock[0] == 1 && p.dsock[1] == 0 && p.dsock[6] == 1 && p.scnt[0] == 1 && p.scnt[1] == 2 && p.scnt[2] == 0 && p.scnt[4] == 0);
        CHECK(p.dstat[2] == kNoSock && p.dstat[3] == kNoSock && p.dstat[4] == kNoSock && p.dstat[5] == (kNoSock | kCtrl));
        CHECK(p.counters[2] == 4 && p.rec[1] == 0 && p.rec[0] == 32 && p.rec[6] == 64 && p.sbase[2] == 96 && p.sbase[5] == 96);
        Plan z(7, 0);
        z.run(b, {}, 8);
        CHECK(z.r == 0 && z.sbase[0] == 0 && z.counters[2] == 7);
        for (int k = 0; k < 7; k++) CHECK((z.dstat[k] & kNoSock) && z.rec[k] == kNone64);
        Batch e((std::vector<Bytes>()));
        Plan y(0, 2);
        y.run(e, bind);
        CHECK(y.r == 0 && y.sbase[0] == 0 && y.sbase[2] == 0 && y.scnt[1] == 0);
    }
    {   // an invalid key: -EINVAL with its index, nothing written
        Batch b({udp(1, 53)});
        const std::vector<uint64_t> badkeys = {key_of(1, 53, A), key_of(0, 0, 0), key_of(17, 53, A) | (1ull << 56),
                                               key_of(6, 80, A) | (1ull << 63)};
        for (uint64_t badkey : badkeys) {
            Plan p(1, 3);
            p.run(b, {bind[0], bind[1], badkey});
            CHECK(p.r == -EINVAL && p.bad == 2 && p.dstat[0] == 0xDEADBEEFu && p.sbase[0] == 0xDEADBEEFull && p.scnt[0] == 0xDEADBEEFu);
        }
        CHECK(check_geometry(8, 65536) == 0 && check_geometry(128, 0) == 0 && check_geometry(8, 65537) == -EINVAL);
        for (uint32_t a : {0u, 1u, 4u, 12u, 24u, 256u, 0x80000000u}) CHECK(check_geometry(a, 1) == -EINVAL);
    }
    // rule 6: the record size
    CHECK(rec_size(0, 8) == 24 && rec_size(1, 8) == 32 && rec_size(8, 8) == 32 && rec_size(9, 8) == 40 && rec_size(0, 128) == 128 &&
          rec_size(104, 128) == 128 && rec_size(105, 128) == 256 && rec_size(65507, 16) == 65536);
}

// The brute-force restatement: for each socket, walk k upward and append.
static void random_batches() {
    std::mt19937 rng(7);
    for (int round = 0; round < 400; round++) {
        const uint32_t S = rng() % 12, n = rng() % 60, align = 8u << (rng() % 5);
        std::vector<uint64_t> bind;
        for (uint32_t s = 0; s < S; s++) bind.push_back(key_of((rng() & 1) ? 6 : 17, 50 + rng() % 4, (rng() & 1) ? A : B));   // duplicates are likely
        std::vector<Bytes> dg;
        std::vector<uint32_t> verdict;
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t P = rng() % 70, port = 50 + rng() % 5, dst = (rng() & 1) ? A : B, hlen = 20 + 4 * (rng() % 3);
            switch (rng() % 8) {
                case 0: dg.push_back(ip(1, Bytes(P, 1), dst)); break;
                case 1: dg.push_back(tcp(rng() % 2, port, dst, 20, (uint8_t)(rng() & 0x1f))); break;
                case 2: { Bytes d = udp(P, port, dst); d.resize(rng() % d.size()); dg.push_back(d); break; }   // truncated
                case 3: case 4: dg.push_back(tcp(P, port, dst, 20 + 4 * (rng() % 11), 0x10, hlen)); break;
                default: dg.push_back(udp(P, port, dst, hlen)); break;
            }
            verdict.push_back((rng() % 9 == 0) ? 0x100u : (rng() % 17 == 0) ? kDgNoRoom : 0x80u);
        }
        Batch b(dg);
        Plan p(n, S);
        const bool use_v = round & 1;
        p.run(b, bind, align, use_v ? verdict.data() : nullptr, 0x100);
        // brute force
        std::vector<uint32_t> st(n), sock(n, kNone32);
        std::vector<uint64_t> size(n, 0);
        uint64_t records = 0;
        for (uint32_t k = 0; k < n; k++) {
            const Cls c = classify(b.off[k], b.len[k], b.bytes, use_v && (verdict[k] & (0x100u | kDgNoRoom)), [&](uint64_t i) { return b.p[i]; });
            st[k] = c.status;
            if (c.status & (kDropped | kNoProto | kShort)) continue;
            for (uint32_t s = 0; s < S && sock[k] == kNone32; s++)
                if (bind[s] == key_of(c.proto, c.dport, c.dst)) sock[k] = s;
            if (sock[k] == kNone32) st[k] |= kNoSock;
            if (st[k] == 0) {
                st[k] = kQueued;
                size[k] = (kRecHdr + c.P + align - 1) / align * align;
                records++;
            }
        }
        CHECK(p.r == (int64_t)records);
        uint64_t at = 0;
        for (uint32_t s = 0; s < S; s++) {
            CHECK(p.sbase[s] == at);
            uint32_t cnt = 0;
            for (uint32_t k = 0; k < n; k++) {
                if (st[k] != kQueued || sock[k] != s) continue;
                CHECK(p.rec[k] == at);
                at += size[k];
                cnt++;
            }
            CHECK(p.scnt[s] == cnt);
        }
        CHECK(p.sbase[S] == at && p.counters[1] == at);
        for (uint32_t k = 0; k < n; k++) {
            CHECK(p.dstat[k] == st[k] && p.dsock[k] == sock[k]);
            if (st[k] != kQueued) CHECK(p.rec[k] == kNone64);
        }
    }
}

int main() {
    rules();
    random_batches();
    if (g_fail) return 1;
    std::printf("dmx_plan_check: ok\n");
    return 0;
}
