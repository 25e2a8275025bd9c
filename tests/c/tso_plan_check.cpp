// tso_plan_check.cpp — stand-alone check of the host planning arithmetic of one-pass TCP segmentation
// (nstack_amd/csrc/tso_plan.hpp, the header txf_engine.cpp plans ip_tx_tso_host with). Built with
// -fsanitize=address,undefined (tests/c/tso_plan_check.mk) and run by tests/test_tso_model.py: every
// arena here is a heap block of exactly the stated size, so a read past a datagram's bytes or past the
// arena's last byte is reported. Without arguments it runs its own cases, prints "tso_plan_check: ok"
// and returns 0. With a file name it plans the batch in that file and prints one line per datagram,
// "status count", and the total, for the test to compare with tests/tso_model.py. The file: u32 n, mtu,
// flags, has_mss; then per datagram u32 len, u32 mss and the bytes.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nstack_amd/csrc/tso_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

struct Arena {   // exactly `bytes` heap bytes
    uint8_t *p;
    uint64_t bytes;
    explicit Arena(uint64_t b) : p((uint8_t *)std::malloc(b ? b : 1)), bytes(b) { std::memset(p, 0xEE, b ? b : 1); }
    ~Arena() { std::free(p); }
};

// A TCP datagram of D bytes: hlen-byte IP header, thl-byte TCP header with `tfl` as its flags byte.
static void put_tcp(uint8_t *h, uint32_t D, uint32_t hlen, uint32_t thl, uint32_t tfl, uint32_t foff = 0, uint32_t proto = 6) {
    std::memset(h, 0, D);
    h[0] = (uint8_t)(0x40u | hlen / 4u);
    h[2] = (uint8_t)(D >> 8);
    h[3] = (uint8_t)D;
    h[6] = (uint8_t)(foff >> 8);
    h[7] = (uint8_t)foff;
    h[8] = 64;
    h[9] = (uint8_t)proto;
    if (D >= hlen + 14u) {
        h[hlen + 12] = (uint8_t)((thl / 4u) << 4);
        h[hlen + 13] = (uint8_t)tfl;
    }
}

static int plan_file(const char *path) {
    std::FILE *f = std::fopen(path, "rb");
    if (!f) return 2;
    uint32_t hd[4];
    if (std::fread(hd, 4, 4, f) != 4) return 2;
    const uint32_t n = hd[0], mtu = hd[1], flags = hd[2], has_mss = hd[3];
    std::vector<uint64_t> off(n);
    std::vector<uint32_t> len(n);
    std::vector<uint16_t> mss(n ? n : 1);
    std::vector<uint8_t> bytes;
    for (uint32_t i = 0; i < n; i++) {
        uint32_t lm[2];
        if (std::fread(lm, 4, 2, f) != 2) return 2;
        off[i] = bytes.size();
        len[i] = lm[0];
        mss[i] = (uint16_t)lm[1];
        bytes.resize(bytes.size() + lm[0]);
        if (lm[0] && std::fread(bytes.data() + off[i], 1, lm[0], f) != lm[0]) return 2;
    }
    std::fclose(f);
    Arena a(bytes.size());
    if (!bytes.empty()) std::memcpy(a.p, bytes.data(), bytes.size());
    std::vector<uint32_t> st(n ? n : 1);
    std::vector<uint64_t> first(n + 1);
    uint64_t bad = 0;
    if (txf::tso_plan_batch(a.p, a.bytes, off.data(), len.data(), has_mss ? mss.data() : nullptr, n, mtu, flags, st.data(),
                            first.data(), &bad))
        return 3;
    for (uint32_t i = 0; i < n; i++)
        std::printf("%u %llu\n", st[i], (unsigned long long)(first[i + 1] - first[i]));
    std::printf("total %llu\n", (unsigned long long)first[n]);
    return 0;
}

int main(int argc, char **argv) {
    using namespace txf;
    if (argc > 1) return plan_file(argv[1]);
    const uint32_t kSeg = kTsoSegmented | kL4CsumSet | (6u << kProtoShift);
    const uint32_t kTcp = 6u << kProtoShift;
    // ---- the count ----
    CHECK(tso_count(65535, 20, 20, 0x10, 0, 0, 1500) == 45 && tso_count(65535, 20, 20, 0x10, 0, 1460, 1500) == 45);
    CHECK(tso_count(8220, 20, 20, 0x18, 0x4000, 0, 1500) == 6 && tso_count(1500, 20, 20, 0x10, 0, 0, 1500) == 0);
    CHECK(tso_count(1501, 20, 20, 0x10, 0, 0, 1500) == 2 && tso_count(1500, 20, 20, 0x10, 0, 1459, 1500) == 2);
    CHECK(tso_count(80, 20, 20, 0x10, 0, 1, 1500) == 40 && tso_count(80, 20, 20, 0x10, 0, 40, 1500) == 0);
    CHECK(tso_count(80, 20, 20, 0x10, 0, 39, 1500) == 2);
    CHECK(tso_count(3000, 20, 16, 0x10, 0, 0, 1500) == 0 && tso_count(3000, 20, 60, 0x10, 0, 0, 1500) == 3);
    CHECK(tso_count(3000, 52, 60, 0x10, 0, 0, 1500) == 3 && tso_count(3000, 56, 60, 0x10, 0, 0, 1500) == 0);
    CHECK(tso_count(3000, 20, 20, 0x12, 0, 0, 1500) == 0 && tso_count(3000, 20, 20, 0x14, 0, 0, 1500) == 0);
    CHECK(tso_count(3000, 20, 20, 0x30, 0, 0, 1500) == 0 && tso_count(3000, 20, 20, 0xd9, 0, 0, 1500) == 3);
    CHECK(tso_count(3000, 20, 20, 0x10, 0x0001, 0, 1500) == 0 && tso_count(3000, 20, 20, 0x10, 0x2000, 0, 1500) == 0);
    CHECK(tso_count(3000, 20, 20, 0x10, 0, 0, 75) == 0 && tso_count(3000, 20, 20, 0x10, 0, 0, 65536) == 0);
    CHECK(tso_count(3000, 54, 60, 0x10, 0, 0, 76) == 0);   // hlen no multiple of 4
    CHECK(tso_count(300, 40, 36, 0x10, 0, 0, 76) == 0 && tso_count(300, 40, 36, 0x10, 0, 0, 77) == 224);   // cap 0 and 1
    CHECK(tso_count(39, 20, 20, 0x10, 0, 1, 1500) == 0 && tso_count(41, 20, 20, 0x10, 0, 1, 1500) == 0);     // L < 20; P = m

    // ---- a batch whose last datagram ends at the arena's last byte ----
    {
        const uint32_t Ds[5] = {3000, 1500, 33, 3000, 100};
        uint64_t total = 0;
        for (uint32_t D : Ds) total += D;
        Arena a(total);
        uint64_t off[5], at = 0;
        uint32_t len[5];
        for (int i = 0; i < 5; i++) {
            off[i] = at;
            len[i] = Ds[i];
            at += Ds[i];
        }
        put_tcp(a.p + off[0], 3000, 20, 20, 0x18);
        put_tcp(a.p + off[1], 1500, 20, 20, 0x10);
        put_tcp(a.p + off[2], 33, 20, 20, 0x10);            // L = 13: bytes 12, 13 of the segment do not exist
        put_tcp(a.p + off[3], 3000, 20, 20, 0x12);          // SYN: fragmented
        put_tcp(a.p + off[4], 100, 20, 20, 0x10);
        const uint16_t mss[5] = {0, 100, 0, 0, 59};
        uint32_t st[5];
        uint64_t first[6], bad = 99;
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, mss, 5, 1500, 0, st, first, &bad) == 0 && bad == 99);
        CHECK(st[0] == kSeg && st[1] == kSeg && st[2] == (kWhole | kL4Short | kTcp));
        CHECK(st[3] == (kFragmented | kL4CsumSet | kTcp) && st[4] == kSeg);
        CHECK(first[0] == 0 && first[1] == 3 && first[2] == 18 && first[3] == 19 && first[4] == 22 && first[5] == 24);
        // mss[0] for all; a null mss
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, mss + 1, 5, 1500, kFlagMssOne, st, first, &bad) == 0);
        CHECK(first[1] == 30 && first[2] == 45 && st[4] == (kWhole | kL4CsumSet | kTcp) && first[5] == 50);
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, nullptr, 5, 1500, 0, nullptr, first, &bad) == 0 && first[5] == 9);
        // one byte less of arena: the last datagram is outside, nothing is written
        uint32_t st2[5] = {7, 7, 7, 7, 7};
        uint64_t first2[6] = {9, 9, 9, 9, 9, 9};
        CHECK(tso_plan_batch(a.p, a.bytes - 1, off, len, mss, 5, 1500, 0, st2, first2, &bad) == -EINVAL && bad == 4);
        CHECK(st2[0] == 7 && st2[4] == 7 && first2[0] == 9 && first2[5] == 9);
    }

    // ---- D of 0..60 bytes with hlen 20 and 40, each in an arena of exactly D bytes ----
    for (uint32_t hlen = 20; hlen <= 40; hlen += 20) {
        for (uint32_t D = 0; D <= 60; D++) {
            Arena a(D);
            if (D >= 20) {
                std::vector<uint8_t> tmp(64 + D);
                put_tcp(tmp.data(), D < hlen + 14 ? hlen + 14 : D, hlen, 20, 0x10);
                tmp[2] = (uint8_t)(D >> 8);
                tmp[3] = (uint8_t)D;
                std::memcpy(a.p, tmp.data(), D);
            }
            const uint64_t off[1] = {0};
            const uint32_t len[1] = {D};
            const uint16_t mss[1] = {1};
            uint32_t st[1] = {0xffu};
            uint64_t first[2] = {9, 9}, bad = 99;
            CHECK(tso_plan_batch(a.p, a.bytes, off, len, mss, 1, 1500, 0, st, first, &bad) == 0);
            const bool hdr = D >= 20 && hlen <= D;
            const uint32_t L = hdr ? D - hlen : 0;
            const uint32_t want = !hdr ? kBadHdr : (L < 20 ? (kWhole | kL4Short | kTcp) : (L <= 21 ? (kWhole | kL4CsumSet | kTcp) : kSeg));
            CHECK(st[0] == want);
            CHECK(first[1] == (!hdr ? 0u : (L <= 21 ? 1u : L - 20u)));
        }
    }

    // ---- refused and other-protocol datagrams keep txf_plan.hpp's words ----
    {
        Arena a(4 * 3000);
        uint64_t off[4] = {0, 3000, 6000, 9000};
        uint32_t len[4] = {3000, 3000, 3000, 3000};
        put_tcp(a.p + 0, 3000, 20, 20, 0x10, 0x2000);       // itself a fragment
        put_tcp(a.p + 3000, 3000, 20, 20, 0x10, 0x4000);    // DF: segmented all the same
        put_tcp(a.p + 6000, 3000, 20, 20, 0x12, 0x4000);    // SYN with DF
        put_tcp(a.p + 9000, 3000, 20, 20, 0x10, 0, 17);     // UDP
        uint32_t st[4];
        uint64_t first[5], bad;
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, nullptr, 4, 1500, kFlagHonorDf, st, first, &bad) == 0);
        CHECK(st[0] == (kRefrag | kTcp) && st[1] == kSeg && st[2] == (kDfDrop | kTcp));
        CHECK(st[3] == (kFragmented | kL4CsumSet | (17u << kProtoShift)) && first[4] == 6);
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, nullptr, 4, 1500, kFlagUdpZero, st, first, &bad) == 0);
        CHECK(st[3] == (kFragmented | (17u << kProtoShift)) && st[2] == (kFragmented | kL4CsumSet | kTcp) && first[4] == 9);
        a.p[9003] ^= 1;   // ip_len != D
        a.p[6000] = 0x35;
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, nullptr, 4, 1500, 0, st, first, &bad) == 0);
        CHECK(st[3] == kBadLen && st[2] == kBadHdr);
    }

    // ---- the largest datagram at the smallest unit ----
    {
        Arena a(65535);
        put_tcp(a.p, 65535, 20, 20, 0x10);
        const uint64_t off[1] = {0};
        const uint32_t len[1] = {65535};
        const uint16_t mss[1] = {1};
        uint32_t st[1];
        uint64_t first[2], bad;
        CHECK(tso_plan_batch(a.p, a.bytes, off, len, mss, 1, 1500, 0, st, first, &bad) == 0 && st[0] == kSeg && first[1] == 65495);
        CHECK(tso_no_room(kSeg) == (kTsoSegmented | kNoRoom | kTcp));
    }

    if (g_fail) return 1;
    std::printf("tso_plan_check: ok\n");
    return 0;
}
