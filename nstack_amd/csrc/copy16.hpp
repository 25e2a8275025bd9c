// copy16.hpp — the realigning 16-lane copy of a row (a quarter-wave): nb bytes from any source address
// to any destination address, every destination byte stored exactly once and no dword read, modified
// and written back. Device code only. mux_kernel.hip is its one user; the copies of rxr_kernel.hip and
// dmx_kernel.hip are the same loop written out in place and stay so (lifting them changed their code
// objects: DESIGN §3.19). This header is the candidate for that later lift.
//
// The destination is cut at its 16-byte grid: the bytes in front of the first line and behind the
// last whole line go out as byte stores (one per lane, fewer than 16 each), the 16-byte pieces
// between them as 16-byte stores, lane j piece j, j + 16, ... with kFlight pieces in flight. A piece's
// source is 16 bytes at any alignment: the four dwords from floor4(source), a fifth where the source
// is not dword-aligned, joined by v_alignbyte. The window of a piece stays inside the dword hull of
// the source range: the caller has checked that the hull may be read.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "row_work.hpp"

namespace copy16 {

using row::gload;
using row::gstore;
using row::kFlight;
using row::kGroup;
using row::u32x4a4;

// Lane j (0..15) of a row: its share of the copy of [s0, s0 + nb) to [dA, dA + nb).
__device__ __forceinline__ void row_copy(uint64_t s0, uint64_t dA, uint32_t nb, int j) {
    // ---- the bytes in front of the destination's first 16-byte line ----
    uint32_t nh = (16u - ((uint32_t)dA & 15u)) & 15u;
    nh = nh < nb ? nh : nb;
    if ((uint32_t)j < nh) gstore<uint8_t>(dA + (uint32_t)j, gload<uint8_t>(s0 + (uint32_t)j));
    // ---- whole 16-byte lines ----
    const uint32_t nblk = (nb - nh) >> 4;
    const uint64_t sb = s0 + nh, db = dA + nh;
    const uint32_t rs = (uint32_t)sb & 3u;
    for (uint32_t b0 = (uint32_t)j; b0 < nblk; b0 += kGroup * kFlight) {
        u32x4a4 x[kFlight];
        uint32_t x4[kFlight];
#pragma unroll
        for (int f = 0; f < kFlight; f++) {
            const uint32_t b = b0 + (uint32_t)(kGroup * f);
            x[f] = u32x4a4{0u, 0u, 0u, 0u};
            x4[f] = 0u;
            if (b < nblk) {
                const uint64_t a4 = (sb + 16ull * b) & ~3ull;
                x[f] = gload<u32x4a4>(a4);
                if (rs) x4[f] = gload<uint32_t>(a4 + 16);
            }
        }
#pragma unroll
        for (int f = 0; f < kFlight; f++) {
            const uint32_t b = b0 + (uint32_t)(kGroup * f);
            if (b < nblk) {
                u32x4a4 y;
                y.x = __builtin_amdgcn_alignbyte(x[f].y, x[f].x, rs);
                y.y = __builtin_amdgcn_alignbyte(x[f].z, x[f].y, rs);
                y.z = __builtin_amdgcn_alignbyte(x[f].w, x[f].z, rs);
                y.w = __builtin_amdgcn_alignbyte(x4[f], x[f].w, rs);
                gstore<u32x4a4>(db + 16ull * b, y);
            }
        }
    }
    // ---- the bytes behind the last whole line ----
    const uint32_t pt = nh + 16u * nblk + (uint32_t)j;
    if (pt < nb) gstore<uint8_t>(dA + pt, gload<uint8_t>(s0 + pt));
}

}  // namespace copy16
