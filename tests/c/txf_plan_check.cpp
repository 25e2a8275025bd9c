// txf_plan_check.cpp — stand-alone check of the host planning arithmetic of one-pass TX framing
// (nstack_amd/csrc/txf_plan.hpp, the header txf_engine.cpp plans with). Built with
// -fsanitize=address,undefined (tests/c/txf_plan_check.mk) and run by tests/test_txf_model.py: every
// arena here is a heap block of exactly the stated size, so a read past a datagram's bytes or past
// the arena's last byte is reported. Prints "txf_plan_check: ok" and returns 0.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../nstack_amd/csrc/txf_plan.hpp"

static int g_fail = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);     \
            g_fail++;                                                       \
        }                                                                   \
    } while (0)

// A datagram header (20 bytes, no options) with ip_len = D unless told otherwise.
static void put_header(uint8_t *h, uint32_t D, uint32_t vhl = 0x45, uint32_t foff = 0) {
    std::memset(h, 0, 20);
    h[0] = (uint8_t)vhl;
    h[2] = (uint8_t)(D >> 8);
    h[3] = (uint8_t)D;
    h[6] = (uint8_t)(foff >> 8);
    h[7] = (uint8_t)foff;
    h[8] = 64;
    h[9] = 17;
}

struct Arena {   // exactly `bytes` heap bytes
    uint8_t *p;
    uint64_t bytes;
    explicit Arena(uint64_t b) : p((uint8_t *)std::malloc(b ? b : 1)), bytes(b) { std::memset(p, 0xEE, b ? b : 1); }
    ~Arena() { std::free(p); }
};

int main() {
    using namespace txf;
    // ---- the arithmetic ----
    CHECK(frag_unit(1500, 20) == 1472 && frag_unit(76, 60) == 8 && frag_unit(76, 20) == 48 && frag_unit(77, 20) == 56);
    CHECK(frame_len(20) == 70 && frame_len(55) == 70 && frame_len(56) == 70 && frame_len(57) == 71 && frame_len(1492) == 1506);
    CHECK(frame_count(1500, 20, 1500) == 1 && frame_count(1501, 20, 1500) == 2 && frame_count(8220, 20, 1500) == 6);
    CHECK(frame_count(65535, 60, 76) == 8185 && frame_count(65535, 20, 1500) == 45);
    CHECK(frame_count(19, 20, 1500) == 0 && frame_count(100, 16, 1500) == 0 && frame_count(100, 20, 75) == 0);
    CHECK(min_slot(1500, 0) == 1514 && min_slot(1500, kFlagFcs) == 1518 && min_slot(76, 0) == 90);
    CHECK(check_geometry(1500, kFlagFcs, 1518) == 0 && check_geometry(1500, kFlagFcs, 1517) == -EINVAL);
    CHECK(check_geometry(75, 0, 4096) == -EINVAL && check_geometry(65536, 0, 1 << 20) == -EINVAL);
    CHECK(check_geometry(1500, 8, 4096) == -EINVAL && check_geometry(65535, 7, 65553) == 0);

    // ---- datagrams that end at the arena's last byte ----
    {
        const uint32_t Ds[4] = {20, 100, 1501, 3000};
        uint64_t total = 0;
        for (uint32_t D : Ds) total += D;
        Arena a(total);
        uint64_t off[4];
        uint32_t len[4];
        uint64_t at = 0;
        for (int i = 0; i < 4; i++) {
            off[i] = at;
            len[i] = Ds[i];
            put_header(a.p + at, Ds[i]);
            at += Ds[i];
        }
        uint32_t st[4];
        uint64_t first[5], bad = 99;
        CHECK(plan_batch(a.p, a.bytes, off, len, 4, 1500, 0, st, first, &bad) == 0 && bad == 99);
        CHECK(st[0] == kWhole && st[1] == kWhole && st[2] == kFragmented && st[3] == kFragmented);
        CHECK(first[0] == 0 && first[1] == 1 && first[2] == 2 && first[3] == 4 && first[4] == 7);
        // one byte less of arena: the last datagram is outside, nothing is written
        uint32_t st2[4] = {7, 7, 7, 7};
        uint64_t first2[5] = {9, 9, 9, 9, 9};
        CHECK(plan_batch(a.p, a.bytes - 1, off, len, 4, 1500, 0, st2, first2, &bad) == -EINVAL && bad == 3);
        CHECK(st2[0] == 7 && st2[3] == 7 && first2[0] == 9 && first2[4] == 9);
        // status may be null
        CHECK(plan_batch(a.p, a.bytes, off, len, 4, 1500, 0, nullptr, first2, &bad) == 0 && first2[4] == 7);
        // slot capacity exact and one short (the comparison ether_tx_frame_host makes)
        CHECK(first[4] <= 7 && !(first[4] <= 6));
    }

    // ---- D of 0..27 bytes, each in an arena of exactly D bytes ----
    for (uint32_t D = 0; D <= 27; D++) {
        Arena a(D);
        if (D >= 20) put_header(a.p, D);
        const uint64_t off[1] = {0};
        const uint32_t len[1] = {D};
        uint32_t st[1] = {0xffu};
        uint64_t first[2] = {9, 9}, bad = 99;
        CHECK(plan_batch(a.p, a.bytes, off, len, 1, 76, 0, st, first, &bad) == 0);
        CHECK(st[0] == (D < 20 ? kBadHdr : kWhole) && first[0] == 0 && first[1] == (D < 20 ? 0u : 1u));
        // the same datagram at the arena's end behind others
        Arena b(64 + D);
        if (D >= 20) put_header(b.p + 64, D, 0x45, 0x4000);
        const uint64_t off2[1] = {64};
        CHECK(plan_batch(b.p, b.bytes, off2, len, 1, 76, kFlagHonorDf, st, first, &bad) == 0);
        CHECK(st[0] == (D < 20 ? kBadHdr : kWhole));
    }

    // ---- the status classes ----
    {
        Arena a(4 * 2000);
        uint64_t off[4] = {0, 2000, 4000, 6000};
        uint32_t len[4] = {1600, 1600, 1600, 1600};
        put_header(a.p + 0, 1600, 0x45, 0x2000);      // a fragment that does not fit
        put_header(a.p + 2000, 1600, 0x45, 0x4000);   // DF
        put_header(a.p + 4000, 1601);                 // ip_len != D
        put_header(a.p + 6000, 1600, 0x35);           // no 0x40
        uint32_t st[4];
        uint64_t first[5], bad;
        CHECK(plan_batch(a.p, a.bytes, off, len, 4, 1500, kFlagHonorDf, st, first, &bad) == 0);
        CHECK(st[0] == kRefrag && st[1] == kDfDrop && st[2] == kBadLen && st[3] == kBadHdr && first[4] == 0);
        CHECK(plan_batch(a.p, a.bytes, off, len, 4, 1500, 0, st, first, &bad) == 0);
        CHECK(st[0] == kRefrag && st[1] == kFragmented && first[4] == 2);
        put_header(a.p + 0, 1600, 0x45, 0x4001);
        CHECK(plan_batch(a.p, a.bytes, off, len, 1, 1500, kFlagHonorDf, st, first, &bad) == 0 && st[0] == (kRefrag | kDfDrop));
    }

    // ---- off + len overflowing 64 bits, off past the arena ----
    {
        Arena a(256);
        put_header(a.p, 100);
        uint64_t off[3] = {0, UINT64_MAX - 10, 0};
        uint32_t len[3] = {100, 100, 100};
        uint32_t st[3] = {7, 7, 7};
        uint64_t first[4] = {9, 9, 9, 9}, bad = 99;
        CHECK(plan_batch(a.p, a.bytes, off, len, 3, 1500, 0, st, first, &bad) == -EINVAL && bad == 1);
        off[1] = UINT64_MAX;
        CHECK(plan_batch(a.p, a.bytes, off, len, 3, 1500, 0, st, first, &bad) == -EINVAL && bad == 1);
        off[1] = 257;
        len[1] = 0;
        CHECK(plan_batch(a.p, a.bytes, off, len, 3, 1500, 0, st, first, &bad) == -EINVAL && bad == 1);
        off[1] = 256;   // an empty datagram at the arena's end is inside it
        CHECK(plan_batch(a.p, a.bytes, off, len, 3, 1500, 0, st, first, &bad) == 0 && st[1] == kBadHdr && first[3] == 2);
        off[1] = 200;
        len[1] = UINT32_MAX;
        st[0] = 7;
        CHECK(plan_batch(a.p, a.bytes, off, len, 3, 1500, 0, st, first, &bad) == -EINVAL && bad == 1 && st[0] == 7);
    }

    // ---- the largest datagram: 8185 slots exact and one short ----
    {
        Arena a(65535);
        std::memset(a.p, 0, 65535);
        put_header(a.p, 65535, 0x4F);
        const uint64_t off[1] = {0};
        const uint32_t len[1] = {65535};
        uint32_t st[1];
        uint64_t first[2], bad;
        CHECK(plan_batch(a.p, a.bytes, off, len, 1, 76, 0, st, first, &bad) == 0 && st[0] == kFragmented && first[1] == 8185);
        const One o = plan_fields(65535, 0x4F, 65535, 0, 76, 0);
        CHECK(o.cnt == 8185 && o.max == 8 && o.hlen == 60 && ((o.cnt - 1) * o.max >> 3) <= 0x1fff);
        CHECK(first[1] <= 8185 && !(first[1] <= 8184));
    }

    if (g_fail) return 1;
    std::printf("txf_plan_check: ok\n");
    return 0;
}
