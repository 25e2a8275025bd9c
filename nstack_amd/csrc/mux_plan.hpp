// mux_plan.hpp — the planning arithmetic of one-pass TX multiplexing (include/nstack_mux.h): what one
// send record is (rules 1-2), the three-step route lookup (rule 3), the header image (rules 5, 7) and
// the build's re-check (rule 8), each stated once for the host plan, the device plan and the build
// kernel; and the host plan of a batch. No HIP: included by mux_kernel.hip (device and host),
// mux_engine.cpp and the stand-alone check tests/c/mux_plan_check.cpp.
#pragma once
#include <errno.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/nstack_mux.h"

#ifdef __HIPCC__
#define MUX_HD __host__ __device__ inline
#else
#define MUX_HD inline
#endif

namespace mux {

constexpr uint32_t kBadRec = 0x001u, kBadSize = 0x002u, kNoTcb = 0x004u, kNoRoute = 0x008u, kNoNeigh = 0x010u, kPlanned = 0x020u,
                   kNoRoom = 0x040u, kBuilt = 0x080u;
constexpr uint32_t kNone32 = 0xffffffffu;
constexpr uint32_t kMaxSocks = 65536u, kMaxRoutes = 256u, kMaxNeigh = 65536u;
constexpr uint32_t kRecHdr = 24u, kImg = 40u, kImgWords = 10u;
constexpr uint32_t kUdpMax = 65506u, kTcpMax = 65495u;
constexpr uint64_t kMaxRecs = 1ull << 30;   // 32-bit ranks

static_assert(sizeof(mux_tcb) == 12 && sizeof(mux_route) == 24 && sizeof(mux_neigh) == 12 && sizeof(txf_l2) == 12,
              "the table layouts of include/nstack_mux.h");

MUX_HD bool key_valid(uint64_t key) { return (key >> 48) == 6u || (key >> 48) == 17u; }   // (bits 56..63 clear with it)
MUX_HD uint32_t key_proto(uint64_t key) { return (uint32_t)(key >> 48); }
MUX_HD uint32_t key_port(uint64_t key) { return (uint32_t)(key >> 32) & 0xffffu; }
MUX_HD uint32_t hl_of(uint32_t proto) { return proto == 17u ? 28u : proto == 6u ? 40u : 0u; }
MUX_HD uint64_t padded(uint32_t len, uint32_t align) { return ((uint64_t)len + align - 1u) & ~(uint64_t)(align - 1u); }
MUX_HD bool has_room(uint64_t at, uint64_t size, uint64_t bytes) { return at <= bytes && size <= bytes - at; }

// Rule 1 on the record at byte offset r of a queue of q_bytes; rd32(i) reads the little-endian dword
// at byte i of the QUEUE and is only called for r <= i < r + 24 <= q_bytes.
struct Rec {
    uint32_t status;   // 0 or kBadRec
    uint32_t dst, dport;
    uint64_t P;
};
template <class Rd32>
MUX_HD Rec read_rec(uint64_t r, uint64_t q_bytes, Rd32 &&rd32) {
    Rec c{kBadRec, 0u, 0u, 0ull};
    if ((r & 7ull) || !has_room(r, kRecHdr, q_bytes)) return c;
    c.P = (uint64_t)rd32(r + 16) | ((uint64_t)rd32(r + 20) << 32);
    if (c.P > q_bytes - r - kRecHdr) return c;
    c.dst = rd32(r + 8);
    c.dport = rd32(r + 12);
    if (c.dport > 0xffffu) return c;   // (a negative int too)
    c.status = 0u;
    return c;
}

// Rule 2: the size bound of the socket's protocol.
MUX_HD bool size_ok(uint32_t proto, uint64_t P) { return proto == 17u ? (P > 0 && P <= kUdpMax) : P <= kTcpMax; }

// Rule 3: ip_route_find_by_network over rt[0, R) in index order; net(i) and mask(i) read entry i.
// Returns the index or kNone32.
template <class Net, class Mask>
MUX_HD uint32_t route_find(uint32_t R, uint32_t dst, Net &&net, Mask &&mask) {
    for (uint32_t i = 0; i < R; i++)
        if (net(i) == dst) return i;
    for (uint32_t i = 0; i < R; i++)
        if (net(i) == (dst & mask(i))) return i;
    for (uint32_t i = 0; i < R; i++)
        if (net(i) == 0u) return i;
    return kNone32;
}

MUX_HD uint32_t bswap32(uint32_t x) { return (x >> 24) | ((x >> 8) & 0xff00u) | ((x << 8) & 0xff0000u) | (x << 24); }

// Rules 5 and 7: the 40-byte image as ten dwords in memory order (little-endian loads of the bytes).
struct Hdr {
    uint32_t proto, P, id, src, dst, sport, dport, seq, ack, flags, win;
};
MUX_HD void make_image(const Hdr &h, uint32_t w[kImgWords]) {
    uint32_t x[kImgWords] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};   // the big-endian words
    x[0] = 0x45000000u | (hl_of(h.proto) + h.P);
    x[1] = ((h.id & 0xffffu) << 16) | 0x4000u;
    x[2] = (64u << 24) | (h.proto << 16);
    x[3] = h.src;
    x[4] = h.dst;
    uint32_t sum = 0u;
    for (int i = 0; i < 5; i++) sum += (x[i] >> 16) + (x[i] & 0xffffu);
    sum = (sum & 0xffffu) + (sum >> 16);
    sum = (sum & 0xffffu) + (sum >> 16);
    x[2] |= ~sum & 0xffffu;
    x[5] = (h.sport << 16) | h.dport;
    if (h.proto == 17u) {
        x[6] = (8u + h.P) << 16;
    } else {
        x[6] = h.seq;
        x[7] = h.ack;
        x[8] = (0x50u << 24) | ((h.flags & 0xffu) << 16) | (h.win & 0xffffu);
    }
    for (uint32_t i = 0; i < kImgWords; i++) w[i] = bswap32(x[i]);
}
MUX_HD uint32_t image_proto(uint32_t w2) { return (w2 >> 8) & 0xffu; }   // byte 9 of the image, from its dword 2

// Rule 8's re-check: whether the planned datagram may be written, whatever the plan arrays say.
MUX_HD bool build_ok(const Rec &c, uint64_t off, uint32_t len, uint32_t w2, uint32_t align, uint64_t dgram_bytes) {
    const uint32_t hl = hl_of(image_proto(w2));
    return c.status == 0u && hl != 0u && (off & (uint64_t)(align - 1u)) == 0ull && (uint64_t)len == hl + c.P &&
           has_room(off, len, dgram_bytes);
}

// 0, or -EINVAL: align is a power of two in 4..128, S <= 65536, R <= 256, N <= 65536.
inline int check_geometry(uint32_t align, uint64_t S, uint64_t R, uint64_t N) {
    if (align < 4u || align > 128u || (align & (align - 1u))) return -EINVAL;
    if (S > kMaxSocks || R > kMaxRoutes || N > kMaxNeigh) return -EINVAL;
    return 0;
}
// Whether sfirst[0 .. S] is 0, monotone, and ends at n.
inline bool sfirst_ok(const uint64_t *sfirst, uint32_t S, uint64_t n) {
    if (S == 0) return n == 0 && (!sfirst || sfirst[0] == 0);
    if (sfirst[0] != 0 || sfirst[S] != n) return false;
    for (uint32_t s = 0; s < S; s++)
        if (sfirst[s] > sfirst[s + 1]) return false;
    return true;
}

// The host plan of a batch (the arrays of include/nstack_mux.h; sfirst_ok holds). Returns the planned
// count. The neighbour lookup is a binary search over (addr, index) sorted: the first of a run is the
// lowest index. tnext and counts may be null.
inline int64_t plan_batch(const uint8_t *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                          const uint64_t *bind, uint32_t S, const mux_tcb *tcb, const mux_route *rt, uint32_t R, const mux_neigh *nb,
                          uint32_t N, uint32_t id0, uint32_t align, uint32_t *mstat, uint64_t *off, uint32_t *len, txf_l2 *l2,
                          uint8_t *himg, uint32_t *tnext, uint64_t *counts) {
    (void)n;   // sfirst[S] (sfirst_ok)
    std::vector<std::pair<uint32_t, uint32_t>> tab;
    tab.reserve(N);
    for (uint32_t i = 0; i < N; i++)
        if (nb[i].valid) tab.push_back({nb[i].addr, i});
    std::sort(tab.begin(), tab.end());
    auto rd32 = [&](uint64_t i) {
        uint32_t v;
        memcpy(&v, q + i, 4);   // (little-endian hosts: the library runs beside a ROCm GPU)
        return v;
    };
    uint64_t at = 0, planned = 0, noroute = 0, noneigh = 0;
    for (uint32_t s = 0; s < S; s++) {
        const uint64_t key = bind[s];
        const uint32_t proto = key_proto(key);
        const bool tcp = key_valid(key) && proto == 6u;
        uint32_t sent = 0u;   // the socket's planned payload bytes so far, mod 2^32
        for (uint64_t k = sfirst[s]; k < sfirst[s + 1]; k++) {
            Rec c = read_rec(rec[k], q_bytes, rd32);
            uint32_t st = key_valid(key) ? c.status : kBadRec, ri = kNone32, ni = kNone32;
            if (!st) {
                if (!size_ok(proto, c.P)) st |= kBadSize;
                if (tcp && !tcb) st |= kNoTcb;
            }
            if (!st) {
                ri = route_find(R, c.dst, [&](uint32_t i) { return rt[i].network; }, [&](uint32_t i) { return rt[i].netmask; });
                if (ri == kNone32) st = kNoRoute;
            }
            if (!st) {
                const auto it = std::lower_bound(tab.begin(), tab.end(), std::make_pair(c.dst, 0u));
                if (it != tab.end() && it->first == c.dst) ni = it->second;
                else st = kNoNeigh;
            }
            uint32_t w[kImgWords] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
            memset(&l2[k], 0, sizeof(txf_l2));
            off[k] = at;
            len[k] = 0u;
            if (!st) {
                st = kPlanned;
                Hdr h{proto, (uint32_t)c.P, (id0 + (uint32_t)planned) & 0xffffu, rt[ri].iface, c.dst, key_port(key), c.dport, 0u, 0u, 0u, 0u};
                if (tcp) {
                    h.seq = tcb[s].seq + sent;
                    h.ack = tcb[s].ack;
                    h.flags = tcb[s].flags;
                    h.win = tcb[s].win;
                    sent += (uint32_t)c.P;
                }
                make_image(h, w);
                len[k] = hl_of(proto) + (uint32_t)c.P;
                at += padded(len[k], align);
                memcpy(l2[k].dst, nb[ni].mac, 6);
                memcpy(l2[k].src, rt[ri].mac, 6);
                planned++;
            }
            noroute += st == kNoRoute;
            noneigh += st == kNoNeigh;
            mstat[k] = st;
            memcpy(himg + k * kImg, w, kImg);
        }
        if (tnext) tnext[s] = tcp && tcb ? tcb[s].seq + sent : 0u;
    }
    if (counts) {
        counts[0] = planned;
        counts[1] = at;
        counts[2] = noroute;
        counts[3] = noneigh;
    }
    return (int64_t)planned;
}

}  // namespace mux
