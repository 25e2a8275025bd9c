// tso_plan.hpp — the planning arithmetic of one-pass TCP segmentation (include/nstack_tso.h, rules
// 1-3 and 6): whether a datagram is segmented, its effective MSS, its frame count and status word,
// and the host plan of a batch. Everything that is not segmented is txf_plan.hpp's, which this header
// calls. No HIP: included by txf_kernel.hip (device and host), txf_engine.cpp and the stand-alone
// check tests/c/tso_plan_check.cpp.
#pragma once
#include "txf_plan.hpp"

namespace txf {

// include/nstack_tso.h: two flags more than nstack_txd.h, one status bit more.
constexpr uint32_t kFlagIdFixed = 0x200u, kFlagMssOne = 0x400u;
constexpr uint32_t kKnownFlagsTso = kKnownFlagsL4 | kFlagIdFixed | kFlagMssOne;
constexpr uint32_t kTsoSegmented = 0x400u;
constexpr uint32_t kTsoMaxHdr = 114u;   // hlen + thl: the 128-byte header image holds 14 + hlen + thl bytes
constexpr uint32_t kTcpFin = 0x01u, kTcpSyn = 0x02u, kTcpRst = 0x04u, kTcpPsh = 0x08u, kTcpUrg = 0x20u, kTcpCwr = 0x80u;

// What one datagram becomes under nstack_tso.h. thl != 0: segmented, o.max is the effective MSS m,
// o.cnt = ceil(P / m) and o.status the whole word of rule 6. thl == 0: everything is nstack_txd.h's:
// o from plan_fields, o.status with the l4_fields bits, fo the checksum field's offset (0: none).
struct TsoOne {
    One o;
    uint32_t thl, fo;
};

// Rule 2 as far as the IP header decides it (the datagram has passed framing rules 1-2): only for
// such a candidate are segment bytes 12 and 13 looked at.
TXF_HD bool tso_candidate(uint32_t D, uint32_t hlen, uint32_t proto, uint32_t ip_foff) {
    return proto == 6u && (ip_foff & 0x3fffu) == 0u && D - hlen >= 20u;
}

// Rules 2-3 for a candidate: the effective MSS m of a datagram that is segmented, 0 for one that is
// not. b12, b13: segment bytes 12 (data offset) and 13 (flags); mss 0: as large as the mtu allows.
TXF_HD uint32_t tso_unit(uint32_t D, uint32_t hlen, uint32_t b12, uint32_t b13, uint32_t mss, uint32_t mtu,
                         uint32_t *thl_out) {
    const uint32_t L = D - hlen, thl = (b12 >> 4) * 4u;
    *thl_out = 0u;
    if (thl < 20u || thl > L || hlen + thl > kTsoMaxHdr) return 0u;
    if (b13 & (kTcpSyn | kTcpRst | kTcpUrg)) return 0u;
    if (mtu < hlen + thl + 1u) return 0u;                                   // cap >= 1
    const uint32_t cap = mtu - hlen - thl, m = (mss && mss < cap) ? mss : cap;
    if (L - thl <= m) return 0u;                                            // rule 3: P > m
    *thl_out = thl;
    return m;
}

// One datagram of D bytes: vhl, ip_len, ip_foff (host order) and proto from its header, looked at
// only when D >= 20; b12 and b13 only for a candidate.
TXF_HD TsoOne tso_fields(uint32_t D, uint32_t vhl, uint32_t ip_len, uint32_t ip_foff, uint32_t proto, uint32_t b12,
                         uint32_t b13, uint32_t mss, uint32_t mtu, uint32_t flags) {
    TsoOne t{plan_fields(D, vhl, ip_len, ip_foff, mtu, flags & kKnownFlags), 0u, 0u};
    if (t.o.status & (kBadHdr | kBadLen)) return t;                         // rule 1
    if (tso_candidate(D, t.o.hlen, proto, ip_foff)) {
        const uint32_t m = tso_unit(D, t.o.hlen, b12, b13, mss, mtu, &t.thl);
        if (m) {
            const uint32_t P = D - t.o.hlen - t.thl;
            t.o.max = m;
            t.o.cnt = (P + m - 1u) / m;
            t.o.status = kTsoSegmented | kL4CsumSet | (6u << kProtoShift);  // rule 6
            t.fo = 16u;
            return t;
        }
    }
    t.o.status |= l4_fields(proto, ip_foff, D - t.o.hlen, t.o.cnt != 0u, flags, &t.fo);
    return t;
}

// A datagram that finds no room (framing rule 9) keeps its class and protocol bits only.
TXF_HD uint32_t tso_no_room(uint32_t status) { return (status & ~(kL4CsumSet | kL4Short)) | kNoRoom; }

// ip_tx_tso_count: the frames of a segmented datagram, 0 for one that is not segmented (or that the
// bounds refuse). ip_foff in host order, tcp_flags the flags byte.
TXF_HD uint32_t tso_count(uint32_t D, uint32_t hlen, uint32_t thl, uint32_t tcp_flags, uint32_t ip_foff, uint32_t mss,
                          uint32_t mtu) {
    if (mtu < kMinMtu || mtu > kMaxMtu || D < 20u || D > 65535u || hlen < 20u || hlen > 60u || (hlen & 3u) || hlen > D)
        return 0u;
    if ((thl & 3u) || thl > 60u || !tso_candidate(D, hlen, 6u, ip_foff)) return 0u;
    uint32_t t = 0u;
    const uint32_t m = tso_unit(D, hlen, (thl >> 2) << 4, tcp_flags, mss, mtu, &t);
    return m ? (D - hlen - thl + m - 1u) / m : 0u;
}

// The host plan of a batch, as txf::plan_batch: status[i] (may be null; the whole word, without
// TXF_NO_ROOM) and first[0..n]. mss may be null; with kFlagMssOne mss[0] serves the batch. Reads
// header bytes 0..9 of datagrams of 20 bytes or more and segment bytes 12, 13 of candidates.
inline int tso_plan_batch(const uint8_t *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                          const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags, uint32_t *status, uint64_t *first,
                          uint64_t *bad) {
    for (uint64_t i = 0; i < n; i++) {
        if (off[i] > dgram_bytes || len[i] > dgram_bytes - off[i]) {
            if (bad) *bad = i;
            return -EINVAL;
        }
    }
    uint64_t k = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *h = dgram + off[i];
        const uint32_t D = len[i];
        TsoOne t{plan_fields(D, 0u, 0u, 0u, mtu, flags & kKnownFlags), 0u, 0u};
        if (D >= 20u) {
            const uint32_t hlen = (h[0] & 0x0fu) * 4u, foff = ((uint32_t)h[6] << 8) | h[7];
            const bool cand = hlen >= 20u && hlen <= D && tso_candidate(D, hlen, h[9], foff);
            t = tso_fields(D, h[0], ((uint32_t)h[2] << 8) | h[3], foff, h[9], cand ? h[hlen + 12u] : 0u,
                           cand ? h[hlen + 13u] : 0u, mss ? mss[(flags & kFlagMssOne) ? 0 : i] : 0u, mtu, flags);
        }
        if (status) status[i] = t.o.status;
        first[i] = k;
        k += t.o.cnt;
    }
    first[n] = k;
    return 0;
}

}  // namespace txf
