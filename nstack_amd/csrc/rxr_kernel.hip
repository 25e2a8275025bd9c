// rxr_kernel.hip — one-pass RX reassembly for gfx950: received Ethernet frames in, IPv4 datagrams
// out, every delivered byte read once and written once (include/nstack_rxr.h has the rules and the
// reference lines they restate).
//
// The build kernel. After the plan every frame is independent: it copies one contiguous source range
// (a whole datagram, a head fragment's header and payload, or another fragment's payload) to
// out + dst[i]. A QUARTER-WAVE takes a frame; rows take runs of kRun consecutive frames from a zeroed
// device counter, as txf_kernel's rows take datagrams.
//   * Two unrelated byte alignments meet. The destination range is cut at the destination's 16-byte
//     grid: up to 15 bytes in front and up to 15 behind go out as byte stores (one per lane), the
//     16-byte pieces between them as 16-byte stores, lane j piece j, j + 16, ... with four pieces in
//     flight. No store touches a byte outside the frame's own destination range (the bytes next to
//     it belong to another row: the neighbouring fragment or datagram), and no dword is read,
//     modified and written back.
//   * A piece's source is 16 bytes at any alignment: the four dwords from floor4(source), a fifth
//     where the source is not dword-aligned, joined by v_alignbyte. The window of a piece is
//     [floor4(s), ceil4(s + 16)) with [s, s + 16) inside the frame, so it stays inside
//     [floor4(frame), ceil4(frame end)) and needs no guard once the frame lies inside the arena
//     (checked per frame). The range ends are byte loads.
//   * A head fragment patches ip_len, ip_foff and the checksum in registers on the way: the
//     checksum comes from a one's-complement sum of its own header dwords with the three fields
//     masked out (lane j holds header dword j), plus the new ip_len, on the memory grid, as
//     txf_kernel's header image does it.
//
//   * rxr_kernel<NT, true> is the same copy for include/nstack_rxd.h: it also sums what it stores, per
//     datagram; rxd_verdict_kernel (behind the plan kernels) turns the sums into L4 verdicts.
//   * rxr_kernel<NT, true, true> is that copy for include/nstack_gro.h: members of a merged TCP
//     datagram behind the first skip both headers, the first patches its own, and
//     rxd_verdict_kernel<true> stores the merged datagram's TCP checksum from the sums.
//
// The plan kernels follow below: classify, insert, link, decide with the block totals, the scan of
// the totals in one workgroup, place, finish. One frame per thread; no workgroup waits for another;
// data passes between the phases only across kernel boundaries. The launchers come in three pieces
// (front, decide, back) so that the coalescing plan (gro_kernel.hip) can put its launches between them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "fcs_crc.hpp"
#include "ones_fold.hpp"
#include "gro_launch.hpp"
#include "row_work.hpp"
#include "rxr_launch.hpp"

namespace rxr {

using ones::fold64;
using ones::row_sum;
using ones::swap16;
using plan::block_scan_excl;
using plan::block_scan_incl;
using row::gload;
using row::gstore;
using row::kFlight;
using row::kGroup;
using row::kRun;
using row::u32x4a4;

constexpr uint32_t kNoFlagPos = 0xffffffffu;

// Rule 7's three fields: the byte at datagram position pos of a head fragment. With fpos (the first
// member of a merged datagram, include/nstack_gro.h rule 4): ip_foff is kept, and the TCP flags byte
// at fpos gets the bits forb.
__device__ __forceinline__ uint32_t patch_byte(uint32_t v, uint32_t pos, uint32_t lenw, uint32_t csum,
                                               uint32_t fpos = kNoFlagPos, uint32_t forb = 0u) {
    if (pos == 2u) return lenw & 0xffu;
    if (pos == 3u) return lenw >> 8;
    if (pos == 6u || pos == 7u) return fpos == kNoFlagPos ? 0u : v;
    if (pos == 10u) return csum & 0xffu;
    if (pos == 11u) return csum >> 8;
    if (pos == fpos) return v | forb;
    return v;
}

__device__ __forceinline__ uint32_t patch_word(uint32_t w, uint32_t p0, uint32_t lenw, uint32_t csum,
                                               uint32_t fpos = kNoFlagPos, uint32_t forb = 0u) {
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const uint32_t nv = patch_byte((w >> (8 * b)) & 0xffu, p0 + (uint32_t)b, lenw, csum, fpos, forb);
        w = (w & ~(0xffu << (8 * b))) | (nv << (8 * b));
    }
    return w;
}

// A byte stored at address a, on the destination memory's 16-bit grid.
__device__ __forceinline__ uint32_t grid_byte(uint64_t a, uint32_t v) { return (a & 1ull) ? v << 8 : v; }

// SUM: the build of include/nstack_rxd.h. Every byte a frame stores is also added to a per-lane
// one's-complement sum on the destination memory's 16-bit grid (the patched header fields as stored);
// the row's folded sum goes to the datagram's accumulator p.dverdict[k] with one atomic add per frame.
// GRO (with SUM): the build of include/nstack_gro.h. A member of a merged datagram that is not its
// first skips its hlen + thl header bytes; the first patches ip_len, the header checksum and the TCP
// flags byte (rule 4; the TCP checksum is the finishing launch's) and marks its datagram's
// accumulator with bit 31.
template <int NT, bool SUM, bool GRO = false>
__global__ __launch_bounds__(NT) void rxr_kernel(RParams p) {
    static_assert(SUM || !GRO, "the coalescing build sums");
    const int j = threadIdx.x & (kGroup - 1);
    const uint32_t T = trailer_of(p.flags);
    const uint64_t arena_bytes = p.arena_bytes;
    // a row takes runs of frames from p.ctr
    row::for_each_item(p.ctr, p.n, [&](uint64_t i) {
        const uint32_t st = p.pstat[i];
        const uint64_t d = p.dst[i];
        uint32_t fin = st;
        if (d != kNone64) {
            const uint32_t k = p.dgi[i], F = p.len[i];
            const uint64_t fo = p.off[i];
            // whatever the plan arrays say, nothing outside the frame is read and nothing outside
            // the datagram's own range inside `out` is written
            bool ok = (uint64_t)k < p.n && (st & (kWhole | kFrag)) && F >= 34u + T && fo <= arena_bytes && F <= arena_bytes - fo;
            uint32_t D = 0u, hlen = 0u, I = 0u;
            uint64_t base = 0;
            const uint64_t start = p.base + fo;
            if (ok) {
                D = p.dlen[k];
                base = p.doff[k];
                hlen = ((uint32_t)gload<uint8_t>(start + 14) & 0x0fu) * 4u;
                I = ((uint32_t)gload<uint8_t>(start + 16) << 8) | (uint32_t)gload<uint8_t>(start + 17);
                ok = hlen >= 20u && hlen <= I && I <= F - 14u - T;
            }
            const bool head = (st & kWhole) || (st & kHead);
            const bool member = GRO && (st & kWhole) && (st & gro::kMerged), first = member && (st & kHead);
            uint32_t skip = head ? 0u : hlen;
            if (GRO && member && ok) {   // the TCP header lies inside the datagram before a byte of it is read
                ok = hlen + 20u <= I;
                if (ok && !first) {
                    const uint32_t thl = ((uint32_t)gload<uint8_t>(start + 14u + hlen + 12u) >> 4) * 4u;
                    ok = thl >= 20u && hlen + thl <= I;
                    skip = hlen + thl;
                }
            }
            const uint32_t nb = I - skip;
            ok = ok && has_room(base, D, p.out_bytes) &&                                  // rule 8: the datagram has room
                 d >= base && d - base <= D && nb <= D - (uint32_t)(d - base);           // and the range lies inside it
            if (!ok) {
                fin |= kNoRoom;
            } else {
                fin |= kDelivered;
                const uint64_t s0 = start + 14u + skip, dA = p.out + d;
                const bool patch = ((st & kFrag) && (st & kHead)) || first;
                const uint32_t fpos = first ? hlen + 13u : kNoFlagPos, forb = first ? gro::flag_bits(st) : 0u;
                uint32_t lenw = 0u, csum = 0u;
                uint32_t acc = 0u;   // SUM: at most 256 lines of eight halves and two bytes per lane, below 2^28
                if (patch) {   // rule 7: the header sum without ip_len, ip_foff and the checksum
                    uint32_t w = 0u;
                    if ((uint32_t)j < hlen / 4u) {
                        const uint64_t a = s0 + 4u * (uint32_t)j, a4 = a & ~3ull;
                        const uint32_t r = (uint32_t)a & 3u;
                        const uint32_t lo = gload<uint32_t>(a4), hi = r ? gload<uint32_t>(a4 + 4) : 0u;
                        w = __builtin_amdgcn_alignbyte(hi, lo, r);
                        if (j < 3 && !(first && j == 1)) w &= 0x0000ffffu;   // a merged datagram keeps ip_foff
                    }
                    lenw = swap16(D);
                    const uint32_t sum = row_sum((w & 0xffffu) + (w >> 16));
                    csum = ~fold64((uint64_t)sum + lenw) & 0xffffu;
                }
                // ---- the bytes in front of the destination's first 16-byte line ----
                uint32_t nh = (16u - ((uint32_t)dA & 15u)) & 15u;
                nh = nh < nb ? nh : nb;
                if ((uint32_t)j < nh) {
                    uint32_t v = gload<uint8_t>(s0 + (uint32_t)j);
                    if (patch) v = patch_byte(v, (uint32_t)j, lenw, csum, fpos, forb);
                    gstore<uint8_t>(dA + (uint32_t)j, (uint8_t)v);
                    if (SUM) acc += grid_byte(dA + (uint32_t)j, v);
                }
                // ---- whole 16-byte lines ----
                const uint32_t nblk = (nb - nh) >> 4;
                const uint64_t sb = s0 + nh, db = dA + nh;
                const uint32_t r = (uint32_t)sb & 3u;
                for (uint32_t b0 = (uint32_t)j; b0 < nblk; b0 += kGroup * kFlight) {
                    u32x4a4 x[kFlight];
                    uint32_t x4[kFlight];
#pragma unroll
                    for (int q = 0; q < kFlight; q++) {
                        const uint32_t b = b0 + (uint32_t)(kGroup * q);
                        x[q] = u32x4a4{0u, 0u, 0u, 0u};
                        x4[q] = 0u;
                        if (b < nblk) {
                            const uint64_t a4 = (sb + 16ull * b) & ~3ull;
                            x[q] = gload<u32x4a4>(a4);
                            if (r) x4[q] = gload<uint32_t>(a4 + 16);
                        }
                    }
#pragma unroll
                    for (int q = 0; q < kFlight; q++) {
                        const uint32_t b = b0 + (uint32_t)(kGroup * q);
                        if (b < nblk) {
                            u32x4a4 y;
                            y.x = __builtin_amdgcn_alignbyte(x[q].y, x[q].x, r);
                            y.y = __builtin_amdgcn_alignbyte(x[q].z, x[q].y, r);
                            y.z = __builtin_amdgcn_alignbyte(x[q].w, x[q].z, r);
                            y.w = __builtin_amdgcn_alignbyte(x4[q], x[q].w, r);
                            const uint32_t pos = nh + 16u * b;
                            if (patch && (pos < 12u || (first && pos <= fpos))) {
                                y.x = patch_word(y.x, pos, lenw, csum, fpos, forb);
                                y.y = patch_word(y.y, pos + 4u, lenw, csum, fpos, forb);
                                y.z = patch_word(y.z, pos + 8u, lenw, csum, fpos, forb);
                                y.w = patch_word(y.w, pos + 12u, lenw, csum, fpos, forb);
                            }
                            gstore<u32x4a4>(db + 16ull * b, y);
                            if (SUM)   // db is 16-byte aligned: eight halves of the memory grid
                                acc += (y.x & 0xffffu) + (y.x >> 16) + (y.y & 0xffffu) + (y.y >> 16) + (y.z & 0xffffu) +
                                       (y.z >> 16) + (y.w & 0xffffu) + (y.w >> 16);
                        }
                    }
                }
                // ---- the bytes behind the last whole line ----
                const uint32_t pt = nh + 16u * nblk + (uint32_t)j;
                if (pt < nb) {
                    uint32_t v = gload<uint8_t>(s0 + pt);
                    if (patch) v = patch_byte(v, pt, lenw, csum, fpos, forb);
                    gstore<uint8_t>(dA + pt, (uint8_t)v);
                    if (SUM) acc += grid_byte(dA + pt, v);
                }
                if (SUM) {
                    // a frame stores at most 65535 bytes, so the row's sum stays below 2^31
                    const uint32_t part = fold64(row_sum(acc));
                    // No overflow of the u32 accumulator: a delivered datagram has at most 8192 frames
                    // (distinct fragment offsets, multiples of 8 below 65536) of at most 0xffff each, and
                    // starts at 0: the total stays below 2^29. Integer adds commute: no order dependence.
                    // GRO: at most 32768 members (distinct seq values of one 32 KiB window) of at most
                    // 0xffff each stay below 2^31; bit 31 is the first member's mark "merged" for the
                    // finishing launch, which has no other way to tell.
                    const uint32_t mark = first ? 0x80000000u : 0u;
                    if (j == 0 && (part | mark)) atomicAdd(p.dverdict + k, part + mark);
                }
            }
        }
        if (j == 0 && p.fstat != nullptr) p.fstat[i] = fin;
    });
}

// ---------------------------------------------------------------------------------------------
// The plan.
// ---------------------------------------------------------------------------------------------
// Frame bytes 12..33 of the frame at `start`, from the dwords of its own dword hull inside the arena.
__device__ __forceinline__ Hdr load_hdr(const RParams &p, uint64_t start, uint32_t F) {
    const uint64_t a = start + 12, a4 = a & ~3ull, he = (start + F + 3ull) & ~3ull;
    const uint32_t r = (uint32_t)a & 3u;
    uint32_t e[7];
#pragma unroll
    for (int q = 0; q < 7; q++) {
        const uint64_t ad = a4 + 4 * q;
        e[q] = (ad >= p.lo4 && ad + 4 <= he && ad + 4 <= p.hi4) ? gload<uint32_t>(ad) : 0u;
    }
    uint32_t w[6];
#pragma unroll
    for (int q = 0; q < 6; q++) w[q] = __builtin_amdgcn_alignbyte(e[q + 1], e[q], r);
    Hdr h;
    h.etype = swap16(w[0] & 0xffffu);
    h.vhl = (w[0] >> 16) & 0xffu;
    h.iplen = swap16(w[1] & 0xffffu);
    h.foff = swap16(w[2] & 0xffffu);
    h.idp = (w[1] >> 16) | ((w[2] >> 24) << 16);
    h.src = (w[3] >> 16) | (w[4] << 16);
    h.dst = (w[4] >> 16) | (w[5] << 16);
    return h;
}

__device__ __forceinline__ bool same_key(const Rec &a, uint32_t src, uint32_t dst, uint32_t idp, uint32_t o) {
    return a.src == src && a.dst == dst && (a.w2 & 0x00ffffffu) == idp && (a.w3 & 0xffffu) == o;
}

// The entry of (key, o), or tsize when there is none. At most tsize probes; the table holds at most
// n <= tsize / 2 claims, so an empty entry ends every miss.
__device__ __forceinline__ uint64_t find(const Scratch &s, uint32_t src, uint32_t dst, uint32_t idp, uint32_t o) {
    uint64_t at = s.tsize;
    plan::probe(s.tsize, plan::mix4(src, dst, idp, o), [&](uint64_t h) {
        const uint32_t c = s.tab[h].claim;
        if (c == 0u) return true;
        if (!same_key(s.rec[c - 1u], src, dst, idp, o)) return false;
        at = h;
        return true;
    });
    return at;
}

// 1. Rules 1-5 and the key record.
__global__ __launch_bounds__(kPlanThreads) void rxr_classify_kernel(RParams p, Scratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n) return;
    // a frame that does not lie inside the arena is a frame of no bytes: RXR_NOT_IPV4, nothing of it is read
    const uint64_t fo = p.off[i];
    const bool inside = fo <= p.arena_bytes && p.len[i] <= p.arena_bytes - fo;
    const uint32_t F = inside ? p.len[i] : 0u;
    const Hdr h = load_hdr(p, p.base + (inside ? fo : 0ull), F);
    const Cls c = classify(F, p.flags, p.verdict != nullptr && (p.verdict[i] & p.drop_mask) != 0u, h);
    p.fstat[i] = c.status;
    Rec rc;
    rc.src = h.src;
    rc.dst = h.dst;
    rc.w2 = (h.idp & 0x00ffffffu) | (c.mf << 24) | ((c.hlen >> 2) << 25) | (groupable(c.status) ? 0x80000000u : 0u);
    rc.w3 = (c.status & kWhole) ? c.I << 16 : (c.o | (c.L << 16));
    s.rec[i] = rc;
    s.headof[i] = kNone32;
}

// 2. Every fragment claims or joins the entry of its (key, o).
__global__ __launch_bounds__(kPlanThreads) void rxr_insert_kernel(RParams p, Scratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n) return;
    const Rec me = s.rec[i];
    if (!(me.w2 & 0x80000000u)) return;
    const uint32_t idp = me.w2 & 0x00ffffffu, o = me.w3 & 0xffffu;
    plan::probe(s.tsize, plan::mix4(me.src, me.dst, idp, o), [&](uint64_t h) {
        const uint32_t old = atomicCAS(&s.tab[h].claim, 0u, (uint32_t)i + 1u);
        if (old != 0u && !same_key(s.rec[old - 1u], me.src, me.dst, idp, o)) return false;
        atomicAdd(&s.tab[h].count, 1u);
        return true;
    });
}

// 3. Every fragment finds its head and its successor and adds itself up on the head's accumulator.
__global__ __launch_bounds__(kPlanThreads) void rxr_link_kernel(RParams p, Scratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n) return;
    const Rec me = s.rec[i];
    if (!(me.w2 & 0x80000000u)) return;
    const uint32_t idp = me.w2 & 0x00ffffffu, o = me.w3 & 0xffffu, L = me.w3 >> 16;
    const bool mf = (me.w2 >> 24) & 1u;
    const uint64_t eh = find(s, me.src, me.dst, idp, 0u);
    if (eh == s.tsize) return;   // no head: headof stays kNone32
    const uint32_t hc = s.tab[eh].claim - 1u;
    s.headof[i] = hc;
    const uint64_t own = o ? find(s, me.src, me.dst, idp, o) : eh;
    bool fault = own == s.tsize || s.tab[own].count != 1u;              // two fragments with the same o
    Acc *a = s.acc + hc;
    if (mf) {
        fault = fault || find(s, me.src, me.dst, idp, o + L) == s.tsize;   // its end is no fragment's o
    } else {
        atomicAdd(&a->lasts, 1u);
        atomicMax(&a->total, o + L);
    }
    atomicAdd(&a->sumL, (unsigned long long)L);
    if (fault) atomicOr(&a->fault, 1u);
}

// 4. Each head decides (rule 6). dgi[i] = 1 on the head frame of a delivered datagram, dst[i] its
// padded length; the blocks' totals of both.
// GRO (include/nstack_gro.h rule 5): a candidate of a coalescible group is a head frame only when it
// is the group's first member, and then with the merged length; every member reads the same settled
// accumulator, so all of them decide alike.
template <bool GRO>
__global__ __launch_bounds__(kPlanThreads) void rxr_decide_kernel(RParams p, Scratch s, gro::GScratch g) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    uint32_t D = 0u, is = 0u;
    if (i < p.n) {
        const uint32_t st = p.fstat[i];
        const Rec me = s.rec[i];
        if (st & kWhole) {
            D = me.w3 >> 16;
            is = 1u;
            if (GRO && (st & gro::kCand)) {
                const gro::GRec gr = g.rec[i];
                const gro::GAcc ga = g.acc[gr.group < p.n ? gr.group : i];   // (every candidate has a group)
                if (gr.group < p.n && gro::coalescible(ga)) {
                    if (gr.first == (uint32_t)i) D = (((gr.w4 >> 16) & 0x0fu) + ((gr.w4 >> 20) & 0x0fu)) * 4u + (uint32_t)ga.sumP;
                    else is = 0u, D = 0u;
                }
            }
        } else if ((st & kHead) && groupable(st) && s.headof[i] == (uint32_t)i) {
            Acc *a = s.acc + i;
            const bool complete = a->fault == 0u && a->lasts == 1u && a->sumL == (unsigned long long)a->total;
            const uint32_t Dd = ((me.w2 >> 25) & 0x0fu) * 4u + a->total;
            uint32_t state = 0u;
            if (complete) state = Dd > 65535u ? 2u : 1u;
            a->state = state;
            if (state == 1u) {
                D = Dd;
                is = 1u;
            }
        }
        if (is) s.acc[i].D = D;
        p.dgi[i] = is;
        p.dst[i] = is ? padded(D, p.align) : 0ull;
    }
    uint64_t tc, tb;
    block_scan_incl<uint64_t>(is, sh, tc);
    block_scan_incl<uint64_t>(is ? padded(D, p.align) : 0ull, sh, tb);
    if (threadIdx.x == 0) {
        s.totc[blockIdx.x] = tc;
        s.totb[blockIdx.x] = tb;
    }
}

// 5. One workgroup: both arrays of block totals become the sums of the blocks in front; counts and
// doff[m].
__global__ __launch_bounds__(kPlanThreads) void rxr_scan_totals_kernel(RParams p, Scratch s, uint64_t nb) {
    __shared__ uint64_t sh[kPlanThreads];
    // both arrays in one loop (the loads of the second overlap the scan of the first), so not two
    // calls of plan::scan_totals
    uint64_t basec = 0, baseb = 0;
    for (uint64_t b0 = 0; b0 < nb; b0 += kPlanThreads) {
        const uint64_t b = b0 + threadIdx.x;
        const uint64_t vc = b < nb ? s.totc[b] : 0ull, vb = b < nb ? s.totb[b] : 0ull;
        uint64_t tc, tb;
        const uint64_t ic = block_scan_incl(vc, sh, tc);
        const uint64_t ib = block_scan_incl(vb, sh, tb);
        if (b < nb) {
            s.totc[b] = basec + ic - vc;
            s.totb[b] = baseb + ib - vb;
        }
        basec += tc;
        baseb += tb;
    }
    if (threadIdx.x == 0) {
        p.doff[basec] = baseb;
        if (p.counts != nullptr) {
            p.counts[0] = basec;
            p.counts[1] = baseb;
        }
    }
}

// 6. Place (rule 8): the head frame of datagram k writes doff[k], dlen[k], dlead[k] and its own dst
// and dgi; every other frame gets "none" here.
__global__ __launch_bounds__(kPlanThreads) void rxr_place_kernel(RParams p, Scratch s) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const uint64_t is = i < p.n ? p.dgi[i] : 0ull, pb = i < p.n ? p.dst[i] : 0ull;
    const uint64_t k = s.totc[blockIdx.x] + block_scan_excl(is, sh);
    const uint64_t at = s.totb[blockIdx.x] + block_scan_excl(pb, sh);
    if (i >= p.n) return;
    if (is) {
        p.dgi[i] = (uint32_t)k;
        p.dst[i] = at;
        p.doff[k] = at;
        p.dlen[k] = s.acc[i].D;
        if (p.dlead != nullptr) p.dlead[k] = (uint32_t)i;
    } else {
        p.dgi[i] = kNone32;
        p.dst[i] = kNone64;
    }
}

// 7. Finish: every fragment takes its group's fate from its head; the others' place was written by
// the launch before and is only read here.
__global__ __launch_bounds__(kPlanThreads) void rxr_finish_kernel(RParams p, Scratch s) {
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    if (i >= p.n) return;
    const Rec me = s.rec[i];
    if (!(me.w2 & 0x80000000u)) return;
    const uint32_t hc = s.headof[i];
    const uint32_t state = hc == kNone32 ? 0u : s.acc[hc].state;
    if (state != 1u) {
        p.fstat[i] |= state == 2u ? kTooBig : kIncomplete;
        return;
    }
    if (hc == (uint32_t)i) return;   // the head: placed
    const uint32_t hl = ((s.rec[hc].w2 >> 25) & 0x0fu) * 4u;
    p.dgi[i] = p.dgi[hc];
    p.dst[i] = p.dst[hc] + hl + (me.w3 & 0xffffu);
}

// ---------------------------------------------------------------------------------------------
// The datagram verdicts (include/nstack_rxd.h). One thread per datagram k < counts[0], launched over
// n threads behind the summing build: dverdict[k] holds the sum of everything the build stored of
// datagram k, on the memory grid. The delivered header is read back from `out` and its sum
// subtracted; what is left is the L4 segment's sum on the memory grid, byte-swapped when the
// segment starts at an odd address (P = swap16(fold(M)), inet_kernel.hip); the pseudo header is
// ones::l4_start's, as in rxv::decode.
// ---------------------------------------------------------------------------------------------
// One's-complement sum of the bytes [a, a + nb) on the memory's 16-bit grid: bytes up to the first
// dword boundary, whole dwords, the bytes behind the last one. Nothing outside the range is read.
__device__ __forceinline__ uint32_t grid_sum(uint64_t a, uint32_t nb) {
    uint32_t s = 0u, q = 0u;
    for (; q < nb && ((a + q) & 3ull); q++) s += grid_byte(a + q, gload<uint8_t>(a + q));
    for (; q + 4u <= nb; q += 4u) {
        const uint32_t w = gload<uint32_t>(a + q);
        s += (w & 0xffffu) + (w >> 16);
    }
    for (; q < nb; q++) s += grid_byte(a + q, gload<uint8_t>(a + q));
    return s;
}

__device__ __forceinline__ uint32_t load_le32(uint64_t a) {   // any alignment
    return (uint32_t)gload<uint8_t>(a) | ((uint32_t)gload<uint8_t>(a + 1) << 8) | ((uint32_t)gload<uint8_t>(a + 2) << 16) |
           ((uint32_t)gload<uint8_t>(a + 3) << 24);
}

// GRO: the finishing launch of include/nstack_gro.h. Bit 31 of the accumulator is the build's mark
// "merged" (its first member was delivered). Such a datagram gets its TCP checksum here: everything
// stored, minus the IP header and the checksum field as the first member brought it, plus the pseudo
// header; the two bytes lie inside the datagram's own range, and the build is complete (kernel
// boundary). Every other datagram is judged as without GRO.
template <bool GRO>
__global__ __launch_bounds__(kPlanThreads) void rxd_verdict_kernel(RParams p) {
    __shared__ unsigned int wg_bad;
    if (threadIdx.x == 0) wg_bad = 0u;
    __syncthreads();
    const uint64_t k = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const uint64_t m = p.counts[0] < p.n ? p.counts[0] : p.n;
    bool is_bad = false;
    if (k < m) {
        const uint32_t D = p.dlen[k];
        const uint64_t at = p.doff[k];
        uint32_t v = 0u;
        if (!has_room(at, D, p.out_bytes)) {
            v = kDgNoRoom;                                    // rule 8 of nstack_rxr.h: nothing was written
        } else if (D >= 20u) {                                // (a plan call's datagram always has its header)
            const uint64_t a = p.out + at;
            const uint32_t hlen = ((uint32_t)gload<uint8_t>(a) & 0x0fu) * 4u;
            if (hlen >= 20u && hlen <= D) {
                const uint32_t proto = gload<uint8_t>(a + 9), L = D - hlen;
                const uint32_t stored = GRO ? p.dverdict[k] & 0x7fffffffu : p.dverdict[k];
                v = proto << kDgProtoShift;
                if (GRO && (p.dverdict[k] >> 31) && L >= 20u) {
                    const uint64_t c = a + hlen + 16u;
                    const uint32_t old = grid_sum(a, hlen) + grid_byte(c, gload<uint8_t>(c)) + grid_byte(c + 1, gload<uint8_t>(c + 1));
                    const uint32_t mem = fold64((uint64_t)fold64(stored) + (0xffffu - fold64(old)));
                    const uint32_t seg = ((a + hlen) & 1ull) ? swap16(mem) : mem;
                    uint32_t none = 0u;
                    const uint32_t ps = ones::l4_start(6u, load_le32(a + 12), load_le32(a + 16), L, 0u, 0u, none);
                    const uint32_t field = ~fold64((uint64_t)ps + seg) & 0xffffu;   // as nstack_txs.h rule 6 stores it
                    gstore<uint8_t>(c, (uint8_t)(field & 0xffu));
                    gstore<uint8_t>(c + 1, (uint8_t)(field >> 8));
                    v = gro::kDgMerged | (6u << kDgProtoShift);
                } else {
                const uint32_t ufield = (proto == 17u && L >= 8u)
                                            ? (uint32_t)gload<uint8_t>(a + hlen + 6) | ((uint32_t)gload<uint8_t>(a + hlen + 7) << 8)
                                            : 0u;
                const uint32_t ps = ones::l4_start(proto, load_le32(a + 12), load_le32(a + 16), L, ufield, kDgL4Short, v);
                if (ps) {
                    // everything stored minus the header, on the memory grid; then on the segment's own
                    const uint32_t mem = fold64((uint64_t)fold64(stored) + (0xffffu - fold64(grid_sum(a, hlen))));
                    const uint32_t seg = ((a + hlen) & 1ull) ? swap16(mem) : mem;
                    v |= kDgL4Checked;
                    if (fold64((uint64_t)ps + seg) != 0xffffu) v |= kDgL4BadCsum;
                }
                }
            }
        }
        p.dverdict[k] = v;
        is_bad = (v & p.bad_mask) != 0u;
    }
    // bad: counted per wave, added once per workgroup
    const uint64_t mb = __ballot(is_bad);
    if (mb != 0 && (threadIdx.x & 63) == 0) atomicAdd(&wg_bad, (unsigned int)__popcll(mb));
    __syncthreads();
    if (threadIdx.x == 0 && wg_bad != 0u && p.bad != nullptr) atomicAdd(p.bad, (unsigned long long)wg_bad);
}

namespace {
std::atomic<int> g_last_route{(int)Route::kNone}, g_last_route_l4{(int)Route::kNone}, g_last_route_gro{(int)Route::kNone};
}
Route last_launch() { return (Route)g_last_route.load(std::memory_order_relaxed); }
Route last_launch_l4() { return (Route)g_last_route_l4.load(std::memory_order_relaxed); }
Route last_launch_gro() { return (Route)g_last_route_gro.load(std::memory_order_relaxed); }

hipError_t launch_build(const RParams &p, int cus, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (!p.n) return hipSuccess;
    if (!p.ctr || (p.gro && !p.dverdict)) return hipErrorInvalidValue;
    // four workgroups per CU at the most, persistent over the frames (a quarter-wave per run of frames)
    const uint64_t rows = kThreads / kGroup, want = (p.n + rows * kRun - 1) / (rows * kRun);
    const uint64_t most = (uint64_t)cus * 4;
    const int grid = (int)(want < most ? want : most);
    if (p.gro) {
        g_last_route_gro.store((int)Route::kGro, std::memory_order_relaxed);
        hipLaunchKernelGGL((rxr_kernel<kThreads, true, true>), dim3(grid), dim3(kThreads), 0, st, p);
    } else if (p.dverdict) {
        g_last_route_l4.store((int)Route::kGeneralL4, std::memory_order_relaxed);
        hipLaunchKernelGGL((rxr_kernel<kThreads, true>), dim3(grid), dim3(kThreads), 0, st, p);
    } else {
        g_last_route.store((int)Route::kGeneral, std::memory_order_relaxed);
        hipLaunchKernelGGL((rxr_kernel<kThreads, false>), dim3(grid), dim3(kThreads), 0, st, p);
    }
    return hipGetLastError();
}

hipError_t launch_verdict(const RParams &p, hipStream_t st) {
    (void)hipGetLastError();
    if (!p.n) return hipSuccess;
    if (!p.dverdict || !p.counts) return hipErrorInvalidValue;
    const uint64_t nb = plan_blocks(p.n);
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    if (p.gro) hipLaunchKernelGGL(rxd_verdict_kernel<true>, dim3((unsigned)nb), dim3(kPlanThreads), 0, st, p);
    else hipLaunchKernelGGL(rxd_verdict_kernel<false>, dim3((unsigned)nb), dim3(kPlanThreads), 0, st, p);
    return hipGetLastError();
}

hipError_t launch_plan_front(const RParams &p, const Scratch &s, hipStream_t st) {
    (void)hipGetLastError();
    const uint64_t nb = plan_blocks(p.n);
    if (!p.n || nb > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)nb), t(kPlanThreads);
    PLAN_LAUNCH(rxr_classify_kernel, g, t, 0, st, p, s);
    PLAN_LAUNCH(rxr_insert_kernel, g, t, 0, st, p, s);
    PLAN_LAUNCH(rxr_link_kernel, g, t, 0, st, p, s);
    return hipSuccess;
}

hipError_t launch_plan_decide(const RParams &p, const Scratch &s, const gro::GScratch *gs, hipStream_t st) {
    (void)hipGetLastError();
    const uint64_t nb = plan_blocks(p.n);
    if (!p.n || nb > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)nb), t(kPlanThreads);
    if (gs) hipLaunchKernelGGL(rxr_decide_kernel<true>, g, t, 0, st, p, s, *gs);
    else hipLaunchKernelGGL(rxr_decide_kernel<false>, g, t, 0, st, p, s, gro::GScratch{});
    return hipGetLastError();
}

hipError_t launch_plan_back(const RParams &p, const Scratch &s, hipStream_t st) {
    (void)hipGetLastError();
    const uint64_t nb = plan_blocks(p.n);
    if (!p.n || nb > 0x7fffffffull) return hipErrorInvalidValue;
    const dim3 g((unsigned)nb), t(kPlanThreads);
    PLAN_LAUNCH(rxr_scan_totals_kernel, dim3(1), t, 0, st, p, s, nb);
    PLAN_LAUNCH(rxr_place_kernel, g, t, 0, st, p, s);
    PLAN_LAUNCH(rxr_finish_kernel, g, t, 0, st, p, s);
    return hipSuccess;
}

// classify, insert, link; decide; the scan of the totals, place, finish
hipError_t launch_plan(const RParams &p, const Scratch &s, hipStream_t st) {
    (void)hipGetLastError();
    if (!p.n) return hipSuccess;
    if (plan_blocks(p.n) > 0x7fffffffull) return hipErrorInvalidValue;
    hipError_t e;
    if ((e = launch_plan_front(p, s, st)) != hipSuccess) return e;
    if ((e = launch_plan_decide(p, s, nullptr, st)) != hipSuccess) return e;
    return launch_plan_back(p, s, st);
}

}  // namespace rxr
