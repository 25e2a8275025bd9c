// txf_plan.hpp — the planning arithmetic of one-pass TX framing (include/nstack_txf.h, rules 1-6
// and 9): what one datagram becomes, and the host plan of a batch with its bounds. No HIP: included
// by txf_kernel.hip (device and host), txf_engine.cpp and the stand-alone check tests/c/txf_plan_check.cpp.
#pragma once
#include <errno.h>
#include <stdint.h>

#ifdef __HIPCC__
#define TXF_HD __host__ __device__ inline
#else
#define TXF_HD inline
#endif

namespace txf {

// Status bits and flags (include/nstack_txf.h).
constexpr uint32_t kWhole = 0x001u, kFragmented = 0x002u, kBadHdr = 0x004u, kBadLen = 0x008u, kRefrag = 0x010u,
                   kDfDrop = 0x020u, kNoRoom = 0x040u;
constexpr uint32_t kFlagFcs = 1u, kFlagHonorDf = 2u, kFlagL2One = 4u, kKnownFlags = 7u;
constexpr uint32_t kMinMtu = 76u, kMaxMtu = 65535u;
// include/nstack_txd.h: framing with L4 checksums takes one flag more and adds these status bits.
constexpr uint32_t kFlagUdpZero = 0x100u, kKnownFlagsL4 = kKnownFlags | kFlagUdpZero;
constexpr uint32_t kL4CsumSet = 0x080u, kL4Short = 0x200u;
constexpr int kProtoShift = 16;

// What one datagram becomes: its status word, frame count, header length and fragment payload unit.
struct One {
    uint32_t status, cnt, hlen, max;
};

// Rule 6: the payload bytes of a full fragment (src/ip.c:220-233, the 8-byte shortfall kept).
TXF_HD uint32_t frag_unit(uint32_t mtu, uint32_t hlen) { return (mtu - hlen - 8u + 7u) & ~7u; }

// Rule 8: the frame of I IP bytes without its FCS (src/linux/ether.c:222-263).
TXF_HD uint32_t frame_len(uint32_t I) { return 14u + (I < 56u ? 56u : I); }

// Rules 1-6 for a datagram of D bytes whose header starts with vhl and holds ip_len and ip_foff
// (host order). vhl, ip_len and ip_foff are looked at only when D >= 20.
TXF_HD One plan_fields(uint32_t D, uint32_t vhl, uint32_t ip_len, uint32_t ip_foff, uint32_t mtu, uint32_t flags) {
    One o{0u, 0u, 0u, 0u};
    const uint32_t hlen = (vhl & 0x0fu) * 4u;
    if (D < 20u || (vhl & 0x40u) != 0x40u || hlen < 20u || hlen > D) {   // rule 1
        o.status = kBadHdr;
        return o;
    }
    o.hlen = hlen;
    if (ip_len != D) {                                                     // rule 2
        o.status = kBadLen;
        return o;
    }
    if (D <= mtu) {                                                        // rule 3
        o.status = kWhole;
        o.cnt = 1u;
        return o;
    }
    if (ip_foff & 0x3fffu) o.status |= kRefrag;                            // rule 4
    if ((flags & kFlagHonorDf) && (ip_foff & 0x4000u)) o.status |= kDfDrop;   // rule 5
    if (o.status) return o;
    o.max = frag_unit(mtu, hlen);                                          // rule 6
    o.cnt = (D - hlen + o.max - 1u) / o.max;
    o.status = kFragmented;
    return o;
}

// include/nstack_txd.h rules 2-4 for a datagram that passed framing rules 1-2: the bits its status
// word gets next to the framing bits, and *fo = the checksum field's offset in the L-byte segment
// (0: no field is written). framed: the datagram becomes frames; ip_foff in host order.
TXF_HD uint32_t l4_fields(uint32_t proto, uint32_t ip_foff, uint32_t L, bool framed, uint32_t flags, uint32_t *fo) {
    const uint32_t bits = proto << kProtoShift;
    *fo = 0u;
    if (!framed || (ip_foff & 0x3fffu)) return bits;                       // rule 2
    const uint32_t need = proto == 6u ? 20u : (proto == 17u ? 8u : (proto == 1u ? 4u : 0u));
    if (!need) return bits;
    if (L < need) return bits | kL4Short;                                  // rule 3
    *fo = proto == 6u ? 16u : (proto == 17u ? 6u : 2u);
    return (proto == 17u && (flags & kFlagUdpZero)) ? bits : (bits | kL4CsumSet);
}

// ether_tx_frame_count: rules 3 and 6 alone; 0 for what rule 1 (or the mtu bound) refuses.
TXF_HD uint32_t frame_count(uint32_t D, uint32_t hlen, uint32_t mtu) {
    if (mtu < kMinMtu || mtu > kMaxMtu || D < 20u || D > 65535u || hlen < 20u || hlen > 60u || hlen > D) return 0u;
    if (D <= mtu) return 1u;
    const uint32_t max = frag_unit(mtu, hlen);
    return (D - hlen + max - 1u) / max;
}

// Rule 9: the smallest slot that holds every frame a call with this mtu can produce.
TXF_HD uint64_t min_slot(uint32_t mtu, uint32_t flags) {
    const uint64_t f = 14ull + mtu;
    return (f < 70ull ? 70ull : f) + ((flags & kFlagFcs) ? 4ull : 0ull);
}

// 0, or -EINVAL for unknown flag bits, an mtu outside [76, 65535] or a slot that is too small.
inline int check_geometry(uint32_t mtu, uint32_t flags, uint64_t slot) {
    if (flags & ~kKnownFlags) return -EINVAL;
    if (mtu < kMinMtu || mtu > kMaxMtu) return -EINVAL;
    if (slot < min_slot(mtu, flags)) return -EINVAL;
    return 0;
}

// The host plan of a batch: status[i] (may be null) and first[0..n] (exclusive prefix sums of the
// frame counts, first[n] the total). Every datagram is checked against the arena first: -EINVAL with
// *bad = the first one outside it, and nothing has been written. Reads bytes 0..7 of datagrams of
// 20 bytes or more only.
inline int plan_batch(const uint8_t *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                      uint32_t mtu, uint32_t flags, uint32_t *status, uint64_t *first, uint64_t *bad) {
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
        const One o = D >= 20u ? plan_fields(D, h[0], ((uint32_t)h[2] << 8) | h[3], ((uint32_t)h[6] << 8) | h[7], mtu, flags)
                               : plan_fields(D, 0u, 0u, 0u, mtu, flags);
        if (status) status[i] = o.status;
        first[i] = k;
        k += o.cnt;
    }
    first[n] = k;
    return 0;
}

}  // namespace txf
