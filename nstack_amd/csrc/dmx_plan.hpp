// dmx_plan.hpp — the planning arithmetic of one-pass RX demultiplexing (include/nstack_dmx.h): what
// one datagram is (rules 1-4 and the lookup key, stated once for the device plan, the host plan and
// the build kernel's re-check), and the host plan of a batch (rules 5-7). No HIP: included by
// dmx_kernel.hip (device and host), dmx_engine.cpp and the stand-alone check tests/c/dmx_plan_check.cpp.
#pragma once
#include <errno.h>
#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#ifdef __HIPCC__
#define DMX_HD __host__ __device__ inline
#else
#define DMX_HD inline
#endif

namespace dmx {

constexpr uint32_t kDropped = 0x001u, kNoProto = 0x002u, kShort = 0x004u, kCtrl = 0x008u, kNoSock = 0x010u, kQueued = 0x020u,
                   kNoRoom = 0x040u, kDelivered = 0x080u;
constexpr uint32_t kDgNoRoom = 0x002u;   // RXD_NO_ROOM (include/nstack_rxd.h)
constexpr uint32_t kNone32 = 0xffffffffu;
constexpr uint64_t kNone64 = ~0ull;
constexpr uint32_t kMaxSocks = 65536u;
constexpr uint32_t kRecHdr = 24u;
constexpr uint64_t kMaxDgs = 1ull << 30;   // 32-bit positions in the partition

// What one datagram is. With none of kDropped, kNoProto, kShort set: its lookup key, and the payload
// [pay, pay + P) inside the datagram. src, sport: the record's source fields (rule 6).
struct Cls {
    uint32_t status;
    uint32_t pay, P;
    uint32_t src, sport, dst, dport, proto;
};

DMX_HD uint64_t key_of(uint32_t proto, uint32_t port, uint32_t addr) {
    return ((uint64_t)proto << 48) | ((uint64_t)port << 32) | addr;
}
DMX_HD bool key_valid(uint64_t key) { return (key >> 48) == 6u || (key >> 48) == 17u; }   // (which also says: bits 56..63 clear)

DMX_HD uint64_t rec_size(uint32_t P, uint32_t align) { return ((uint64_t)kRecHdr + P + align - 1u) & ~(uint64_t)(align - 1u); }

DMX_HD bool has_room(uint64_t at, uint64_t size, uint64_t bytes) { return at <= bytes && size <= bytes - at; }

// Rules 1-4 for the datagram of D bytes at byte offset `at` of an arena of out_bytes; rd(i) reads
// byte i of the ARENA and is only called for at <= i < at + D <= out_bytes. `bad_verdict`: rule 1's
// verdict test.
template <class Rd>
DMX_HD Cls classify(uint64_t at, uint32_t D, uint64_t out_bytes, bool bad_verdict, Rd &&rd) {
    Cls c{kDropped, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (!has_room(at, D, out_bytes) || bad_verdict || D < 20u) return c;           // rule 1
    const uint32_t hlen = ((uint32_t)rd(at) & 15u) * 4u;
    if (hlen < 20u || hlen > D) return c;
    c.proto = rd(at + 9);
    if (c.proto != 6u && c.proto != 17u) {                                         // rule 2
        c.status = kNoProto;
        return c;
    }
    const uint32_t L = D - hlen;
    const uint64_t seg = at + hlen;
    uint32_t hl4 = 8u;                                                             // rule 3
    if (c.proto == 6u) {                                                           // rule 4
        hl4 = L >= 20u ? ((uint32_t)rd(seg + 12) >> 4) * 4u : 0u;
        if (hl4 < 20u) hl4 = L + 1u;
    }
    if (hl4 > L) {
        c.status = kShort;
        return c;
    }
    c.pay = hlen + hl4;
    c.P = L - hl4;
    c.status = 0u;
    if (c.proto == 6u && (c.P == 0u || ((uint32_t)rd(seg + 13) & 0x06u))) c.status = kCtrl;   // SYN 0x02, RST 0x04
    auto be32 = [&](uint64_t a) {
        return ((uint32_t)rd(a) << 24) | ((uint32_t)rd(a + 1) << 16) | ((uint32_t)rd(a + 2) << 8) | (uint32_t)rd(a + 3);
    };
    c.src = be32(at + 12);
    c.dst = be32(at + 16);
    c.sport = ((uint32_t)rd(seg) << 8) | (uint32_t)rd(seg + 1);
    c.dport = ((uint32_t)rd(seg + 2) << 8) | (uint32_t)rd(seg + 3);
    return c;
}

// 0, or -EINVAL: align is a power of two in 8..128, S <= 65536.
inline int check_geometry(uint32_t align, uint64_t S) {
    if (align < 8u || align > 128u || (align & (align - 1u))) return -EINVAL;
    if (S > kMaxSocks) return -EINVAL;
    return 0;
}

// The host plan of a batch of n datagrams (the arrays of include/nstack_dmx.h). -EINVAL with *bad = the
// first invalid bind key, and nothing written. Returns the record count. The lookup is a binary
// search over the keys sorted by (key, index): the first of a run is the lowest index.
inline int64_t plan_batch(const uint8_t *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                          const uint32_t *dverdict, uint64_t n, const uint64_t *bind, uint32_t S, uint32_t drop_mask,
                          uint32_t align, uint32_t *dstat, uint32_t *dsock, uint64_t *rec, uint64_t *sbase, uint32_t *scnt,
                          uint64_t *bad, uint64_t *counters = nullptr) {
    for (uint32_t s = 0; s < S; s++) {
        if (!key_valid(bind[s])) {
            if (bad) *bad = s;
            return -EINVAL;
        }
    }
    std::vector<std::pair<uint64_t, uint32_t>> tab(S);
    for (uint32_t s = 0; s < S; s++) tab[s] = {bind[s], s};
    std::sort(tab.begin(), tab.end());
    std::vector<uint64_t> bytes((size_t)S + 1, 0ull);   // bytes[s + 1]: the record bytes of socket s
    std::vector<uint32_t> size(n, 0u);
    uint64_t records = 0, nosock = 0, dropped = 0;
    for (uint32_t s = 0; s < S; s++) scnt[s] = 0u;
    for (uint64_t k = 0; k < n; k++) {
        const Cls c = classify(doff[k], dlen[k], out_bytes, dverdict && (dverdict[k] & (drop_mask | kDgNoRoom)),
                               [&](uint64_t i) { return out[i]; });
        uint32_t st = c.status, sock = kNone32;
        if (!(st & (kDropped | kNoProto | kShort))) {                              // rule 5
            const auto it = std::lower_bound(tab.begin(), tab.end(), std::make_pair(key_of(c.proto, c.dport, c.dst), 0u));
            if (it != tab.end() && it->first == key_of(c.proto, c.dport, c.dst)) sock = it->second;
            else st |= kNoSock;
        }
        if (st == 0u) {                                                            // rule 6
            st = kQueued;
            size[k] = (uint32_t)rec_size(c.P, align);
            bytes[sock + 1] += size[k];
            scnt[sock]++;
            records++;
        }
        nosock += (st & kNoSock) != 0u;
        dropped += (st & kDropped) != 0u;
        dstat[k] = st;
        dsock[k] = sock;
        rec[k] = kNone64;
    }
    sbase[0] = 0;                                                                  // rule 7
    for (uint32_t s = 0; s < S; s++) sbase[s + 1] = sbase[s] + bytes[s + 1];
    std::vector<uint64_t> at(sbase, sbase + S);
    for (uint64_t k = 0; k < n; k++) {
        if (!(dstat[k] & kQueued)) continue;
        rec[k] = at[dsock[k]];
        at[dsock[k]] += size[k];
    }
    if (counters) {
        counters[0] = records;
        counters[1] = sbase[S];
        counters[2] = nosock;
        counters[3] = dropped;
    }
    return (int64_t)records;
}

}  // namespace dmx
