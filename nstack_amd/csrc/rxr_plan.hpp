// rxr_plan.hpp — the planning arithmetic of one-pass RX reassembly (include/nstack_rxr.h): what one
// frame is (rules 1-5, stated once for the device plan, the host plan and the build kernel's
// re-check), and the host plan of a batch (rules 6-8). No HIP: included by rxr_kernel.hip (device
// and host), rxr_engine.cpp and the stand-alone check tests/c/rxr_plan_check.cpp.
#pragma once
#include <errno.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#ifdef __HIPCC__
#define RXR_HD __host__ __device__ inline
#else
#define RXR_HD inline
#endif

namespace rxr {

// Status bits and flags (include/nstack_rxr.h).
constexpr uint32_t kWhole = 0x001u, kFrag = 0x002u, kHead = 0x004u, kDropped = 0x008u, kNotIpv4 = 0x010u,
                   kBadHdr = 0x020u, kBadLen = 0x040u, kFragBad = 0x080u, kIncomplete = 0x100u, kTooBig = 0x200u,
                   kNoRoom = 0x400u, kDelivered = 0x800u;
// Datagram verdict bits (include/nstack_rxd.h; the L4 bits have nstack_rxv.h's values).
constexpr uint32_t kDgNoRoom = 0x002u, kDgL4Checked = 0x080u, kDgL4BadCsum = 0x100u, kDgL4Short = 0x200u, kDgProtoShift = 16u;
constexpr uint32_t kFlagTrailer = 1u, kKnownFlags = 1u;
constexpr uint32_t kNone32 = 0xffffffffu;
constexpr uint64_t kNone64 = ~0ull;
constexpr uint64_t kMaxFrames = 1ull << 30;   // 32-bit claims, and a table of fewer than 2^32 entries

// The header fields the rules look at. etype, iplen and foff in host order; src, dst and idp
// (ip_id | ip_proto << 16) as the bytes lie in the header, read as little-endian words. A field whose
// bytes lie outside the frame is never looked at (fields_of leaves it 0).
struct Hdr {
    uint32_t etype, vhl, iplen, foff, src, dst, idp;
};

// What one frame is.
struct Cls {
    uint32_t status;
    uint32_t hlen, I;   // valid once no bit of rules 1-3 is set
    uint32_t o, L, mf;  // kFrag
};

RXR_HD uint32_t trailer_of(uint32_t flags) { return (flags & kFlagTrailer) ? 4u : 0u; }

// The nstack_rxv.h rules 2-4 (RXV_RUNT, not RXV_IPV4, RXV_IP_BAD_HDR), stated once for reassembly:
// 0, kNotIpv4 or kBadHdr.
RXR_HD uint32_t header_rules(uint32_t F, uint32_t T, const Hdr &h) {
    if (F < 14u + T) return kNotIpv4;                                     // rxv rule 2
    if (h.etype != 0x0800u) return kNotIpv4;                              // rxv rule 3
    const uint32_t P = F - 14u - T, hlen = (h.vhl & 0x0fu) * 4u;
    if (P < 20u || (h.vhl & 0x40u) != 0x40u || hlen < 20u || hlen > P) return kBadHdr;   // rxv rule 4
    return 0u;
}

// Rules 1-5 for a frame of F bytes.
RXR_HD Cls classify(uint32_t F, uint32_t flags, bool dropped, const Hdr &h) {
    Cls c{0u, 0u, 0u, 0u, 0u, 0u};
    if (dropped) {                                                        // rule 1
        c.status = kDropped;
        return c;
    }
    const uint32_t T = trailer_of(flags);
    if ((c.status = header_rules(F, T, h))) return c;                     // rule 2
    const uint32_t P = F - 14u - T;
    c.hlen = (h.vhl & 0x0fu) * 4u;
    c.I = h.iplen;
    if (c.I < c.hlen || c.I > P) {                                        // rule 3
        c.status = kBadLen;
        return c;
    }
    if ((h.foff & 0x3fffu) == 0u) {                                       // rule 4
        c.status = kWhole;
        return c;
    }
    c.status = kFrag;                                                     // rule 5
    c.o = (h.foff & 0x1fffu) * 8u;
    c.L = c.I - c.hlen;
    c.mf = (h.foff & 0x2000u) ? 1u : 0u;
    if (c.L == 0u || c.o + c.L + 20u > 65535u) c.status |= kFragBad;
    else if (c.o == 0u) c.status |= kHead;
    return c;
}

// A fragment that can join a group.
RXR_HD bool groupable(uint32_t status) { return (status & kFrag) && !(status & kFragBad); }

RXR_HD uint64_t padded(uint32_t D, uint32_t align) { return ((uint64_t)D + align - 1u) & ~(uint64_t)(align - 1u); }

// Rule 8: a datagram of D bytes placed at `at` lies inside out_bytes.
RXR_HD bool has_room(uint64_t at, uint32_t D, uint64_t out_bytes) { return at <= out_bytes && D <= out_bytes - at; }

// 0, or -EINVAL for unknown flag bits or an align that is no power of two in 1..128.
inline int check_geometry(uint32_t flags, uint32_t align) {
    if (flags & ~kKnownFlags) return -EINVAL;
    if (align == 0u || align > 128u || (align & (align - 1u))) return -EINVAL;
    return 0;
}

// The header fields of a frame of F bytes in host memory: bytes outside [0, F - T) are not read.
inline Hdr fields_of(const uint8_t *f, uint32_t F, uint32_t T) {
    Hdr h{0u, 0u, 0u, 0u, 0u, 0u, 0u};
    if (F < 14u + T) return h;
    h.etype = ((uint32_t)f[12] << 8) | f[13];
    if (F - 14u - T < 20u) return h;
    const uint8_t *p = f + 14;
    h.vhl = p[0];
    h.iplen = ((uint32_t)p[2] << 8) | p[3];
    h.foff = ((uint32_t)p[6] << 8) | p[7];
    h.idp = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[9] << 16);
    h.src = (uint32_t)p[12] | ((uint32_t)p[13] << 8) | ((uint32_t)p[14] << 16) | ((uint32_t)p[15] << 24);
    h.dst = (uint32_t)p[16] | ((uint32_t)p[17] << 8) | ((uint32_t)p[18] << 16) | ((uint32_t)p[19] << 24);
    return h;
}

// The host plan of a batch (the arrays of include/nstack_rxr.h; dlead may be null). Every frame is
// checked against the arena first: -EINVAL with *bad = the first one outside it, and nothing has
// been written. Returns m. Groups by sorting the fragments by (key, o, index).
inline int64_t plan_batch(const uint8_t *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                          uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat,
                          uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint64_t *bad) {
    for (uint64_t i = 0; i < n; i++) {
        if (off[i] > arena_bytes || len[i] > arena_bytes - off[i]) {
            if (bad) *bad = i;
            return -EINVAL;
        }
    }
    const uint32_t T = trailer_of(flags);
    struct Fr {
        uint32_t src, dst, idp, o, L, mf, hlen;
        uint64_t i;
    };
    std::vector<Fr> fr;
    std::vector<uint32_t> D(n, 0u);        // the datagram length, on head frames of delivered datagrams
    std::vector<uint64_t> headof(n, kNone64);
    std::vector<uint32_t> rel(n, 0u);      // a delivered frame's offset inside its datagram
    for (uint64_t i = 0; i < n; i++) {
        const Hdr h = fields_of(arena + off[i], len[i], T);
        const Cls c = classify(len[i], flags, verdict && (verdict[i] & drop_mask), h);
        fstat[i] = c.status;
        if (c.status & kWhole) {
            D[i] = c.I;
            headof[i] = i;
        } else if (groupable(c.status)) {
            fr.push_back(Fr{h.src, h.dst, h.idp, c.o, c.L, c.mf, c.hlen, i});
        }
    }
    std::sort(fr.begin(), fr.end(), [](const Fr &a, const Fr &b) {
        if (a.src != b.src) return a.src < b.src;
        if (a.dst != b.dst) return a.dst < b.dst;
        if (a.idp != b.idp) return a.idp < b.idp;
        if (a.o != b.o) return a.o < b.o;
        return a.i < b.i;
    });
    for (size_t a = 0; a < fr.size();) {                                  // rule 6: one group per key
        size_t e = a + 1;
        while (e < fr.size() && fr[e].src == fr[a].src && fr[e].dst == fr[a].dst && fr[e].idp == fr[a].idp) e++;
        uint32_t heads = 0, lasts = 0, total = 0;
        uint64_t sum = 0;
        bool ok = true;
        for (size_t q = a; q < e; q++) {
            const Fr &f = fr[q];
            heads += f.o == 0u;
            sum += f.L;
            if (q > a && fr[q - 1].o == f.o) ok = false;                  // two fragments with the same o
            if (!f.mf) {
                lasts++;
                total = f.o + f.L;
            } else {                                                      // its end is another fragment's o
                const uint32_t end = f.o + f.L;
                size_t lo = a, hi = e;
                while (lo < hi) {
                    const size_t mid = (lo + hi) / 2;
                    if (fr[mid].o < end) lo = mid + 1;
                    else hi = mid;
                }
                if (lo == e || fr[lo].o != end) ok = false;
            }
        }
        ok = ok && heads == 1u && lasts == 1u && sum == total;
        const Fr &hd = fr[a];   // sorted by o: the head where there is one
        if (!ok) {
            for (size_t q = a; q < e; q++) fstat[fr[q].i] |= kIncomplete;
        } else if (hd.hlen + total > 65535u) {
            for (size_t q = a; q < e; q++) fstat[fr[q].i] |= kTooBig;
        } else {
            D[hd.i] = hd.hlen + total;                                    // rule 7
            for (size_t q = a; q < e; q++) {
                headof[fr[q].i] = hd.i;
                rel[fr[q].i] = fr[q].o ? hd.hlen + fr[q].o : 0u;
            }
        }
        a = e;
    }
    uint64_t m = 0, at = 0;                                               // rule 8
    for (uint64_t i = 0; i < n; i++) {
        if (headof[i] != i) continue;
        doff[m] = at;
        dlen[m] = D[i];
        if (dlead) dlead[m] = (uint32_t)i;
        dgi[i] = (uint32_t)m;
        at += padded(D[i], align);
        m++;
    }
    doff[m] = at;
    for (uint64_t i = 0; i < n; i++) {
        if (headof[i] == kNone64) {
            dgi[i] = kNone32;
            dst[i] = kNone64;
        } else {
            dgi[i] = dgi[headof[i]];
            dst[i] = doff[dgi[i]] + rel[i];
        }
    }
    return (int64_t)m;
}
}  // namespace rxr
