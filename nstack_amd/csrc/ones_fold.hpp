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

}  // namespace ones
