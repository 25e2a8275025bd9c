// gro_plan.hpp — the planning arithmetic of one-pass RX coalescing (include/nstack_gro.h): what a
// candidate segment is (rule 2) and when two segments' headers agree (rule 3d), stated once for the
// device plan, the host plan and the build kernel's re-check, and the host plan of a batch (rules
// 3-5) on top of rxr::plan_batch. No HIP: included by gro_kernel.hip and rxr_kernel.hip (device and
// host), rxr_engine.cpp and the stand-alone check tests/c/gro_plan_check.cpp.
#pragma once
#include <errno.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "rxr_plan.hpp"

namespace gro {

// Status bits and the datagram verdict bit (include/nstack_gro.h).
constexpr uint32_t kCand = 0x1000u, kMerged = 0x2000u, kFin = 0x4000u, kPsh = 0x8000u;
constexpr uint32_t kDgMerged = 0x400u;
// TCP flag bits (segment byte 13).
constexpr uint32_t kTcpFin = 0x01u, kTcpSyn = 0x02u, kTcpRst = 0x04u, kTcpPsh = 0x08u, kTcpUrg = 0x20u, kTcpCwr = 0x80u;
constexpr uint32_t kWinShift = 15u, kWin = 1u << kWinShift;   // the 32 KiB window of absolute sequence space
constexpr uint32_t kMaxI = kWin;                             // rule 2: the design limit on a candidate's ip_len
constexpr uint32_t kMaxMembers = kWin;                       // distinct seq values of one window, P >= 1

// What rule 2 reads of a candidate. ports: the four port bytes as they lie (a little-endian word).
struct Seg {
    uint32_t ports, seq, thl, P, tflags;
};

// Rule 2 for an RXR_WHOLE frame whose datagram has ip_proto `proto`, header length hlen and length I.
// byte(q) is datagram byte q; only bytes inside [hlen, hlen + 14) are asked for, and only once
// I - hlen >= 20 is known.
template <class B>
RXR_HD bool candidate(uint32_t proto, uint32_t hlen, uint32_t I, B byte, Seg &s) {
    if (proto != 6u || I > kMaxI || I < hlen + 20u) return false;
    const uint32_t L = I - hlen;
    s.thl = ((uint32_t)byte(hlen + 12u) >> 4) * 4u;
    if (s.thl < 20u || s.thl > L) return false;
    s.P = L - s.thl;
    if (s.P < 1u) return false;
    s.tflags = byte(hlen + 13u);
    if (s.tflags & (kTcpSyn | kTcpRst | kTcpUrg)) return false;
    s.ports = (uint32_t)byte(hlen) | ((uint32_t)byte(hlen + 1u) << 8) | ((uint32_t)byte(hlen + 2u) << 16) |
              ((uint32_t)byte(hlen + 3u) << 24);
    s.seq = ((uint32_t)byte(hlen + 4u) << 24) | ((uint32_t)byte(hlen + 5u) << 16) | ((uint32_t)byte(hlen + 6u) << 8) |
            (uint32_t)byte(hlen + 7u);
    return true;
}

// Rule 3d for two candidates that both have header lengths hlen and thl (the caller has compared
// them): every IP header byte but 2-3, 4-5 and 10-11, and every TCP header byte but 4-7, the FIN,
// PSH and CWR bits of byte 13, and 16-17. a(q), b(q): datagram byte q of either, q < hlen + thl.
template <class A, class B>
RXR_HD bool compatible(A a, B b, uint32_t hlen, uint32_t thl) {
    for (uint32_t q = 0; q < hlen; q++) {
        if ((q >= 2u && q <= 5u) || q == 10u || q == 11u) continue;
        if (a(q) != b(q)) return false;
    }
    for (uint32_t q = 0; q < thl; q++) {
        if ((q >= 4u && q <= 7u) || q == 16u || q == 17u) continue;
        const uint32_t mask = q == 13u ? 0xffu & ~(kTcpFin | kTcpPsh | kTcpCwr) : 0xffu;
        if (((uint32_t)a(hlen + q) & mask) != ((uint32_t)b(hlen + q) & mask)) return false;
    }
    return true;
}

// The status bits a merged datagram's first member gets from the last member's TCP flags (rule 4).
RXR_HD uint32_t last_bits(uint32_t last_tflags) {
    return ((last_tflags & kTcpFin) ? kFin : 0u) | ((last_tflags & kTcpPsh) ? kPsh : 0u);
}
// The bits the build ORs into the first member's TCP flags byte, from its status word.
RXR_HD uint32_t flag_bits(uint32_t status) { return ((status & kFin) ? kTcpFin : 0u) | ((status & kPsh) ? kTcpPsh : 0u); }

// The host plan of a batch (the arrays of include/nstack_rxr.h; dlead may be null): rxr::plan_batch,
// then rules 2-5 of include/nstack_gro.h over its RXR_WHOLE frames. Returns m, or -EINVAL with
// *bad = the first frame outside the arena and nothing written. Groups by sorting the candidates by
// (flow, seq, index).
inline int64_t plan_batch(const uint8_t *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                          uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat,
                          uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint64_t *bad) {
    std::vector<uint32_t> own_lead;
    if (!dlead) {
        own_lead.resize(n ? n : 1);
        dlead = own_lead.data();
    }
    const int64_t m0 = rxr::plan_batch(arena, arena_bytes, off, len, n, flags, verdict, drop_mask, align, fstat, dst, dgi, doff,
                                       dlen, dlead, bad);
    if (m0 <= 0) return m0;
    struct Cd {
        uint32_t src, dst, ports, seq, P, hlen, thl, tflags;
        uint64_t i;
    };
    auto ip_of = [&](uint64_t i) { return arena + off[i] + 14; };
    std::vector<Cd> c;
    for (uint64_t i = 0; i < n; i++) {                                     // rule 2
        if (!(fstat[i] & rxr::kWhole)) continue;
        const uint8_t *ip = ip_of(i);
        const rxr::Hdr h = rxr::fields_of(arena + off[i], len[i], rxr::trailer_of(flags));
        const uint32_t hlen = (h.vhl & 0x0fu) * 4u;
        Seg s{0u, 0u, 0u, 0u, 0u};
        if (!candidate(h.idp >> 16, hlen, h.iplen, [&](uint32_t q) { return ip[q]; }, s)) continue;
        fstat[i] |= kCand;
        c.push_back(Cd{h.src, h.dst, s.ports, s.seq, s.P, hlen, s.thl, s.tflags, i});
    }
    std::sort(c.begin(), c.end(), [](const Cd &a, const Cd &b) {
        if (a.src != b.src) return a.src < b.src;
        if (a.dst != b.dst) return a.dst < b.dst;
        if (a.ports != b.ports) return a.ports < b.ports;
        if (a.seq != b.seq) return a.seq < b.seq;
        return a.i < b.i;
    });
    std::vector<uint64_t> firstof(n, rxr::kNone64);   // a merged member's first member
    std::vector<uint32_t> rel(n, 0u), newD(n, 0u);    // its offset inside the datagram; on the first: D
    bool any = false;
    for (size_t a = 0; a < c.size();) {                                    // rule 3: one group per (flow, window)
        size_t e = a + 1;
        while (e < c.size() && c[e].src == c[a].src && c[e].dst == c[a].dst && c[e].ports == c[a].ports &&
               (c[e].seq >> kWinShift) == (c[a].seq >> kWinShift))
            e++;
        if (e - a >= 2) {
            const Cd &f = c[a];   // sorted by seq: the first member
            const uint8_t *fip = ip_of(f.i);
            bool ok = true;
            uint32_t lasts = 0, last_end = 0, last_flags = 0;
            uint64_t sum = 0;
            for (size_t q = a; q < e; q++) {
                const Cd &x = c[q];
                sum += x.P;
                if (q > a && c[q - 1].seq == x.seq) ok = false;                                   // (a)
                const uint32_t end = x.seq + x.P;                                                  // mod 2^32
                bool succ = false;
                if ((end >> kWinShift) == (x.seq >> kWinShift)) {                                  // a member of this group
                    size_t lo = a, hi = e;
                    while (lo < hi) {
                        const size_t mid = (lo + hi) / 2;
                        if (c[mid].seq < end) lo = mid + 1;
                        else hi = mid;
                    }
                    succ = lo < e && c[lo].seq == end;
                }
                if (!succ) {                                                                        // (b)
                    lasts++;
                    last_end = end;
                    last_flags = x.tflags;
                } else if (x.tflags & (kTcpFin | kTcpPsh)) {                                       // (e)
                    ok = false;
                }
                if (q > a) {
                    if (x.tflags & kTcpCwr) ok = false;                                            // (e)
                    const uint8_t *xip = ip_of(x.i);
                    if (x.hlen != f.hlen || x.thl != f.thl ||                                      // (d)
                        !compatible([&](uint32_t p) { return fip[p]; }, [&](uint32_t p) { return xip[p]; }, f.hlen, f.thl))
                        ok = false;
                }
            }
            ok = ok && lasts == 1u && sum == (uint64_t)(uint32_t)(last_end - f.seq);               // (b), (c)
            if (ok) {                                                                               // rule 4
                any = true;
                newD[f.i] = f.hlen + f.thl + (uint32_t)sum;
                for (size_t q = a; q < e; q++) {
                    firstof[c[q].i] = f.i;
                    rel[c[q].i] = q == a ? 0u : f.hlen + f.thl + (c[q].seq - f.seq);
                    fstat[c[q].i] |= kMerged;
                }
                fstat[f.i] |= rxr::kHead | last_bits(last_flags);
            }
        }
        a = e;
    }
    if (!any) return m0;
    // rule 5: the members behind the first give up their datagrams; everything else keeps its order
    const uint64_t m_old = (uint64_t)m0;
    std::vector<uint64_t> odoff(doff, doff + m_old + 1), odst(dst, dst + n);
    std::vector<uint32_t> odlen(dlen, dlen + m_old), odlead(dlead, dlead + m_old), odgi(dgi, dgi + n), newk(m_old, rxr::kNone32);
    uint64_t m = 0, at = 0;
    for (uint64_t k = 0; k < m_old; k++) {
        const uint64_t lead = odlead[k];
        if (firstof[lead] != rxr::kNone64 && firstof[lead] != lead) continue;
        const uint32_t D = firstof[lead] == lead ? newD[lead] : odlen[k];
        newk[k] = (uint32_t)m;
        doff[m] = at;
        dlen[m] = D;
        dlead[m] = (uint32_t)lead;
        at += rxr::padded(D, align);
        m++;
    }
    doff[m] = at;
    for (uint64_t i = 0; i < n; i++) {
        if (odgi[i] == rxr::kNone32) continue;
        if (firstof[i] != rxr::kNone64) {
            dgi[i] = newk[odgi[firstof[i]]];
            dst[i] = doff[dgi[i]] + rel[i];
        } else {
            dgi[i] = newk[odgi[i]];
            dst[i] = doff[dgi[i]] + (odst[i] - odoff[odgi[i]]);
        }
    }
    return (int64_t)m;
}

}  // namespace gro
