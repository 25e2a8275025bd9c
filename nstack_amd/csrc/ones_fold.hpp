// ones_fold.hpp — the one's-complement fold helpers of the checksum kernels (inet_kernel.hip and,
// through frame_walk.hpp, rxv_kernel.hip, txs_kernel.hip and txf_kernel.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ones {

__device__ __forceinline__ uint32_t swap16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

// End-around-carry fold to [0, 0xffff]; 0 only for x == 0.
__device__ __forceinline__ uint32_t fold64(uint64_t x) {
    uint64_t y = (x & 0xffffffffull) + (x >> 32);
    y = (y & 0xffffu) + (y >> 16);
    y = (y & 0xffffu) + (y >> 16);
    return (uint32_t)((y & 0xffffu) + (y >> 16));
}

// Sum over a 16-lane row; every lane ends with the row's sum.
__device__ __forceinline__ uint32_t row_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);   // quad [1,0,3,2]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);   // quad [2,3,0,1]
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x141, 0xF, 0xF, false);  // row_half_mirror
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x140, 0xF, 0xF, false);  // row_mirror
    return v;
}

// include/nstack_rxv.h rule 8, stated once for the validator (rxv::decode) and the reassembly verdict
// (rxd_verdict_kernel): what the check of an L-byte L4 segment of `proto` starts from. src and dst are
// the header's address words as they lie (little-endian reads), ufield the UDP checksum field.
//   ps: the accumulator start plus the pseudo header; 0 = no L4 checksum to verify.
//   tcp_checksum(ntohl(src), ntohl(dst), seg, L): htonl() of both gives back the words as they lie;
//   udp_checksum(seg, L, src, dst): the raw in_addr_t words; ip_checksum(msg, L) for ICMP.
// ip_checksum and tcp_checksum start at 0xffff, udp_checksum adds the non-zero protocol word, so the
// folded total is never 0 and the reference returns 0 exactly when it is 0xffff.
// A segment too short for its protocol sets `short_bit` (the callers' L4_SHORT) in `bits`.
__device__ __forceinline__ uint32_t l4_start(uint32_t proto, uint32_t src, uint32_t dst, uint32_t L, uint32_t ufield,
                                             uint32_t short_bit, uint32_t &bits) {
    uint32_t ps = 0u;
    const uint32_t l16 = swap16(L);
    const uint32_t a4 = (src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16);
    if (proto == 6u) {
        if (L < 20u) bits |= short_bit;
        else ps = 0xffffu + a4 + 0x0600u + l16;
    } else if (proto == 17u) {
        if (L < 8u) bits |= short_bit;
        else if (ufield != 0u) ps = a4 + 0x1100u + l16;
    } else if (proto == 1u) {
        if (L < 4u) bits |= short_bit;
        else ps = 0xffffu;
    }
    return ps;
}

}  // namespace ones
