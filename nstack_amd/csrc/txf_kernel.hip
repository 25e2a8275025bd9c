// txf_kernel.hip — one-pass TX framing for gfx950: IPv4 datagrams in, wire-ready Ethernet frames
// out, every payload byte read once and written once (include/nstack_txf.h has the rules and the
// reference lines they restate). The frame walk is rxv_kernel's (frame_walk.hpp, fcs_crc.hpp): a
// QUARTER-WAVE per datagram with an outer loop over its fragments; within a frame lane j owns the
// 96-byte chunk that ends 96 j bytes before the frame END, longer frames are walked in 1536-byte
// segments counted from the frame end. A full fragment at mtu 1500 (1506 bytes) is one pass.
//
// What is new here:
//   * The frame does not exist yet. Frame position q >= 14 + hlen is datagram byte
//     q - 14 + j * max (the header length cancels), so a lane loads its chunk from the datagram at
//     the SOURCE's alignment and aligns it to the frame-end grid (v_alignbyte), as the other kernels
//     do. The 14 + hlen bytes in front come from a header image held in registers: lane l of the
//     row holds dwords l and l + 16 of the frame's first 128 bytes, built once per datagram from
//     its first dwords and the MAC record, with ip_len, ip_foff and the checksum zeroed. Their sum
//     is reduced once per datagram; per fragment the three fields are ORed in:
//       csum = ~fold(header sum + ip_len + ip_foff)            (one's-complement, memory grid)
//     The one or two lanes whose chunk holds header bytes fetch those dwords by ds_bpermute and
//     merge them by byte mask. Padding (I < 56) and the bytes in front of the frame are masked to
//     zero; the CRC chains then run over the words exactly as they will be stored.
//   * Two byte alignments meet. The destination of a chunk is out + k * slot + position, whose
//     low two bits change from slot to slot when slot is no multiple of 4. The chunk's words are
//     aligned a second time, to the DESTINATION's dword grid: dword t of a lane holds chunk bytes
//     [4 t - rd, 4 t - rd + 4), the bytes in front of a chunk come from the neighbouring lane's last
//     word (one ds_bpermute) or, for lane 15, from the previous segment's lane 0 (carried). Stores
//     are 16-byte stores of four dwords on that grid.
//   * Edges. The neighbouring slot belongs to another quarter-wave, so the frame's first and last
//     partial dword are written by byte stores: the up to three bytes in front of the first whole
//     dword are MAC bytes every lane knows; the up to three bytes behind the last whole dword go
//     out together with the four FCS bytes, one byte per lane.
//   * Work. Datagrams differ by three orders of magnitude (one frame or 8185), so rows are not
//     given datagrams i mod the grid: a row takes a run of kRun consecutive datagrams from a
//     zeroed device counter (one atomicAdd per wave for all its rows that ran dry, no waiting on
//     anybody) and comes back for the next run when it is done.
// Reads stay inside [lo4, hi4) of the datagram arena: a chunk window that crosses its edge is
// loaded dword by dword under a guard (the batch's first and last datagram at most).
//
// The walk is written once, frame_walk<FCSW, Mode, NT>: txf_kernel is its plain form, txd_kernel the
// form that also fills every datagram's TCP / UDP / ICMP checksum (include/nstack_txd.h), tso_kernel
// that form with eligible TCP datagrams cut into MSS segments instead of fragments
// (include/nstack_tso.h); the comment in front of frame_walk has what each adds.
//
// The plan kernels (status and exclusive prefix sums of the frame counts) follow below: counts and
// block totals, a one-workgroup scan of the totals, the add; no workgroup waits for another.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>

#include "fcs_crc.hpp"
#include "fcs_tables.hpp"
#include "frame_walk.hpp"
#include "row_work.hpp"
#include "txf_launch.hpp"

namespace txf {

using fcs::kChunkBytes;
using fcs::kChunkWords;
using fcs::kGroup;
using fcs::kSegBytes;
using fcs::u32x4a4;
using row::gstore;
using row::kRun;
static_assert(fcs::kGroup == row::kGroup, "a quarter-wave per datagram");
using rxv::fold64;
using rxv::keep_range;
using rxv::row_get;
using rxv::row_sum;
using rxv::swap16;
using rxv::xor_field;

// What the L4 variant (include/nstack_txd.h) keeps besides; empty for the plain framer, whose
// structures and code stay what they were.
template <bool L4>
struct DgL4 {};
template <>
struct DgL4<true> {
    uint32_t ps;       // accumulator start plus pseudo header; 0: nothing is summed
    uint32_t qf;       // frame position of the checksum field in fragment fidx; 0: no field is written
    uint32_t fidx;     // the fragment that holds the field, walked last; cnt - 1 without a field
    uint32_t old;      // the field's content in the datagram (memory grid)
    uint32_t mac;      // folded sum of frame bytes [0, 14)
    uint32_t proto;
};
template <bool L4>
struct PosL4 {};
template <>
struct PosL4<true> {
    uint32_t t;        // the frames of the datagram walked before this one
    bool pre;          // a visit that only sums (a field frame of several segments)
};

// What the segmenting variant (include/nstack_tso.h) keeps besides; empty for the other two.
template <bool TSO>
struct DgTso {};
template <>
struct DgTso<true> {
    uint32_t thl;      // the TCP header's bytes; 0: not segmented, the datagram takes the L4 path
    uint32_t hb;       // the bytes of every frame that come from the image behind the MAC header: hlen (+ thl)
    uint32_t seq0;     // the datagram's sequence number (host order)
    uint32_t id0;      // its ip_id (host order)
    uint32_t tfl;      // its TCP flags byte
};
template <bool TSO>
struct FrameTso {};
template <>
struct FrameTso<true> {
    uint32_t f1;       // img1 with this frame's TCP fields (hlen >= 32 puts them there)
};

constexpr bool l4_of(Mode m) { return m != Mode::kPlain; }
constexpr bool tso_of(Mode m) { return m == Mode::kTso; }

// A datagram that becomes frames (uniform over the row but for the image).
template <Mode M>
struct Dg : DgL4<l4_of(M)>, DgTso<tso_of(M)> {
    uint64_t src;      // the address frame position 0 of fragment 0 maps to: datagram address - 14
    uint64_t slot0;    // its first slot
    uint32_t D, hlen, cnt;
    uint32_t max;      // 0: TXF_WHOLE
    uint32_t img0, img1;   // lane l: dwords l and l + 16 of the frame's first 128 bytes; ip_len, ip_foff, checksum zero
    uint32_t hsum;     // folded sum of the image's header bytes [14, 14 + hlen)
    uint32_t keep;     // the datagram's own ip_len | ip_foff << 16, as they lie in memory (TXF_WHOLE)
};

template <Mode M>
struct Frame : FrameTso<tso_of(M)> {
    uint64_t fo;       // address of the frame's first byte
    uint64_t src;      // the address frame position 0 maps to in the datagram arena
    uint32_t F, I, m;  // frame bytes, IP bytes, segments
    uint32_t f0;       // img0 with this frame's ip_len, ip_foff and checksum
};

template <Mode M>
__device__ __forceinline__ Frame<M> idle_frame() {   // what a row without work holds: one segment of nothing
    Frame<M> f{};
    f.m = 1u;
    return f;
}

template <Mode M>
struct Pos : PosL4<l4_of(M)> {
    uint32_t jf, k;    // fragment, segment
    bool act;
    Dg<M> g;
    Frame<M> fr;
};

struct Chunk {
    u32x4a4 x[6];
    uint32_t x6;
    uint32_t r;        // source address of the chunk's first byte & 3
};

template <Mode M>
__device__ __forceinline__ int rel_of(const Pos<M> &c, int j) {   // frame position of the chunk's first byte
    return (int)rxv::rel_of(c.fr.F, c.fr.m, c.k, j);
}

// Mode::kTso: dword d of a segment's header image part that changes from frame to frame, T = 14 + hlen
// the frame position of the TCP header (T & 3 == 2): tcp_seqno at T + 4 (sw: its four bytes as they
// lie), the flags byte at T + 13, the checksum at T + 16. All ones in, the mask of these fields out.
__device__ __forceinline__ uint32_t tcp_words(uint32_t d, uint32_t T, uint32_t sw, uint32_t fl, uint32_t cs) {
    const uint32_t ds = (T + 4u) >> 2, df = (T + 13u) >> 2, dc = (T + 16u) >> 2;
    return (d == ds ? sw << 16 : 0u) | (d == ds + 1u ? sw >> 16 : 0u) | (d == df ? fl << 24 : 0u) | (d == dc ? cs << 16 : 0u);
}

// L4 (include/nstack_txd.h): the same walk, plus the TCP / UDP / ICMP checksum of every datagram.
//   * The sum. A frame's words are summed as they will be stored (rxv::add_sums, the frame END's
//     word grid; a frame of odd length has its folded sum swapped, as rxv::reduce_sums does for a
//     whole frame; fragment offsets and 14 + hlen are even, so the frame start's grid is the
//     segment's). Each lane keeps one running sum per datagram; the row's sum is reduced once, at the
//     datagram's last frame. What is not segment leaves again: frame bytes [0, 14) of every frame
//     (their sum is known from the image), nothing for the IP header, whose stored bytes sum to
//     0xffff, nothing for the padding, which is zero. The field's old content leaves too.
//   * The order. The value is known after the datagram's last byte but lies near its front, so a
//     row walks the fragment that holds the field (fo / max) LAST. A field frame of one segment has
//     all its words in registers when the sum is complete: new ^ old is XORed into them before the
//     CRC chains run and before anything is stored, as txs_kernel does. A field frame of several
//     segments (jumbo mtu) is visited twice: the first visit only sums (its loads are the only cost;
//     no CRC result is kept and nothing is stored), the second is the ordinary one and XORs the
//     delta into the chunk that holds the field. Every byte is stored once, by the lane that owns
//     it, with its final value: no late store, and no order between stores is relied on.
//
// TSO (include/nstack_tso.h): the L4 walk, in which an eligible TCP datagram whose payload exceeds its
// MSS m is cut into frames of m payload bytes instead of fragments. What differs for such a datagram:
//   * The image holds the TCP header too (hb = hlen + thl bytes behind the MAC header), with ip_len,
//     ip_id, the IP checksum, tcp_seqno, the flags byte and the TCP checksum zero. frame_of ORs the
//     frame's own values into BOTH image dwords (f0, f1): from hlen 32 on the TCP fields lie in dwords
//     16 and up. The payload of frame s starts s m bytes further on in the datagram.
//   * The checksum belongs to the frame. Every frame is a field frame: its sum is reduced at its own
//     end (on its own grid: m may be odd, so the parity swap is per frame), the pseudo header takes
//     the frame's thl + plen, and the value is XORed into the words before the CRC chains and the
//     stores. Frames are walked in order. A frame of several 1536-byte segments takes the sum-only
//     first visit: at mtu > 1522 that is every full frame of a segmented datagram.
// Every statement of this mode sits under `if constexpr (TSO)`.
template <bool FCSW, Mode M, int NT>
__device__ __forceinline__ void frame_walk(FParams p) {
    constexpr bool L4 = l4_of(M), TSO = tso_of(M);
    using Dg = txf::Dg<M>;
    using Pos = txf::Pos<M>;
    using Frame = txf::Frame<M>;
    // TSO: the datagram is segmented; the bytes the image gives every frame behind the MAC header
    auto seg_of = [](const Dg &g) -> bool {
        if constexpr (TSO) return g.thl != 0u;
        else return false;
    };
    auto hb_of = [](const Dg &g) -> uint32_t {
        if constexpr (TSO) return g.hb;
        else return g.hlen;
    };
    __shared__ __attribute__((aligned(16))) uint8_t lds[FCSW ? fcs::kLdsBytes : 16];
    if (FCSW) fcs::stage_tables<NT>(rxv::tables_of(p.blob), lds);
    const int lane = threadIdx.x & 63, j = lane & (kGroup - 1);
    uint32_t tb0, tb1;
    fcs::table_bases(lane, tb0, tb1);
    const uint32_t lanebase = fcs::kLdsLane | ((uint32_t)(lane & 31) * 4u);
    row::Run run;   // this row's run of datagrams, taken from p.ctr

    auto frame_of = [&](const Dg &g, uint32_t jf) -> Frame {
        Frame f;
        const bool whole = g.max == 0u;
        const uint32_t hb = hb_of(g);
        const uint32_t B = g.D - hb, at = jf * g.max;
        const uint32_t plen = B - at < g.max ? B - at : g.max;
        f.I = whole ? g.D : hb + plen;
        const uint32_t fo16 = (jf + 1u < g.cnt ? 0x2000u : 0u) | (at >> 3);
        const uint32_t lenw = whole ? (g.keep & 0xffffu) : swap16(f.I);
        uint32_t foffw = whole ? (g.keep >> 16) : swap16(fo16);
        uint32_t idw = 0u;   // TSO: a segment's own ip_id; its ip_foff stays as it lies
        if constexpr (TSO) {
            if (seg_of(g)) {
                foffw = g.keep >> 16;
                idw = swap16((g.id0 + ((p.flags & kFlagIdFixed) ? 0u : jf)) & 0xffffu);
            }
        }
        const uint32_t csum = ~fold64((uint64_t)g.hsum + lenw + foffw + idw) & 0xffffu;   // rule 7
        f.f0 = g.img0 | (j == 4 ? lenw | (idw << 16) : 0u) | (j == 5 ? foffw : 0u) | (j == 6 ? csum : 0u);
        if constexpr (TSO) {
            f.f1 = g.img1;
            if (seg_of(g)) {   // tcp_seqno and the flags of segment jf (nstack_tso.h rule 4)
                const uint32_t T = 14u + g.hlen, sw = __builtin_bswap32(g.seq0 + at);
                uint32_t fl = g.tfl;
                if (jf + 1u < g.cnt) fl &= ~(kTcpFin | kTcpPsh);
                if (jf) fl &= ~kTcpCwr;
                f.f0 |= tcp_words((uint32_t)j, T, sw, fl, 0u);
                f.f1 |= tcp_words((uint32_t)j + 16u, T, sw, fl, 0u);
            }
        }
        f.F = frame_len(f.I);
        f.m = (f.F + (uint32_t)kSegBytes - 1u) / (uint32_t)kSegBytes;
        f.fo = p.out + (g.slot0 + jf) * p.slot;
        f.src = g.src + at;
        return f;
    };

    // Datagram i: rules 1-6 and 9, its status word, and (where it becomes frames) its header image.
    auto load_dg = [&](uint64_t i) -> Dg {
        Dg g{};
        const uint64_t a = p.dg + p.off[i];
        const uint32_t D = p.len[i], r = (uint32_t)a & 3u;
        const uint64_t a4 = a & ~3ull, he = (a + D + 3ull) & ~3ull;
        const uint64_t ha = a4 + 4ull * (uint32_t)j;
        uint32_t h0 = 0u, h1 = 0u;   // dwords j and j + 16 from floor4(datagram), inside it and the arena
        if (ha >= p.lo4 && ha + 4 <= he && ha + 4 <= p.hi4) h0 = fcs::gload<uint32_t>(ha);
        if (ha + 64 >= p.lo4 && ha + 68 <= he && ha + 68 <= p.hi4) h1 = fcs::gload<uint32_t>(ha + 64);
        const uint32_t e0 = row_get(h0, 0u), e1 = row_get(h0, 1u), e2 = row_get(h0, 2u);
        const uint32_t w0 = __builtin_amdgcn_alignbyte(e1, e0, r);   // vhl, tos, ip_len
        const uint32_t w4 = __builtin_amdgcn_alignbyte(e2, e1, r);   // id, ip_foff
        // the datagram's dwords e and e + 1 of that grid (128 bytes from floor4 on)
        auto hget = [&](int e) -> uint32_t {
            const uint32_t v0 = row_get(h0, (uint32_t)e & 15u), v1 = row_get(h1, (uint32_t)e & 15u);
            return e < 0 ? 0u : (e < 16 ? v0 : v1);
        };
        One o;
        g.slot0 = p.first[i];
        uint32_t l4bits = 0u, fo = 0u;
        if constexpr (TSO) {   // nstack_tso.h rules 1-3 and 6 (tso_plan.hpp); the rest as below
            const uint32_t w8 = __builtin_amdgcn_alignbyte(row_get(h0, 3u), e2, r);   // ttl, proto, checksum
            g.proto = (w8 >> 8) & 0xffu;
            const uint32_t b = (w0 & 0x0fu) * 4u + 12u + r;   // segment bytes 12, 13: looked at for candidates only
            const uint32_t tw = __builtin_amdgcn_alignbyte(hget((int)(b >> 2) + 1), hget((int)(b >> 2)), b & 3u);
            uint32_t mss = 0u;
            if (p.mss != nullptr) mss = p.mss[(p.flags & kFlagMssOne) ? 0ull : i];
            const TsoOne t = tso_fields(D, w0 & 0xffu, swap16(w0 >> 16), swap16(w4 >> 16), g.proto, tw & 0xffu,
                                        (tw >> 8) & 0xffu, mss, p.mtu, p.flags);
            o = t.o;
            fo = t.fo;
            g.thl = t.thl;
            if (o.cnt && (g.slot0 > p.slots || o.cnt > p.slots - g.slot0)) {   // rule 9
                o.status = tso_no_room(o.status);
                o.cnt = 0u;
            }
            l4bits = o.status & kL4CsumSet;
        } else {
            o = plan_fields(D, w0 & 0xffu, swap16(w0 >> 16), swap16(w4 >> 16), p.mtu, p.flags);
            if (o.cnt && (g.slot0 > p.slots || o.cnt > p.slots - g.slot0)) {   // rule 9
                o.status |= kNoRoom;
                o.cnt = 0u;
            }
        }
        if constexpr (L4 && !TSO) {   // proto; segment length, field offset
            const uint32_t w8 = __builtin_amdgcn_alignbyte(row_get(h0, 3u), e2, r);   // ttl, proto, checksum
            g.proto = (w8 >> 8) & 0xffu;
            if (!(o.status & (kBadHdr | kBadLen)))
                l4bits = l4_fields(g.proto, swap16(w4 >> 16), D - o.hlen, o.cnt != 0u, p.flags, &fo);
        }
        if (j == 0 && p.status != nullptr) p.status[i] = o.status | l4bits;
        g.cnt = o.cnt;
        if (!o.cnt) return g;
        g.D = D;
        g.hlen = o.hlen;
        g.max = o.max;
        g.src = a - 14ull;
        g.keep = (w0 >> 16) | (w4 & 0xffff0000u);
        // frame dword d holds frame bytes 4 d .. 4 d + 3 = datagram bytes 4 d - 14 ..: dwords
        // d - 4 + c and the next of the datagram's grid, shifted by (2 + r) & 3
        const uint32_t c = (2u + r) >> 2, sh = (2u + r) & 3u;
        const int e = j - 4 + (int)c;
        g.img0 = __builtin_amdgcn_alignbyte(hget(e + 1), hget(e), sh);
        g.img1 = __builtin_amdgcn_alignbyte(hget(e + 17), hget(e + 16), sh);
        if (j < 3) {   // the MAC pair, rule 8
            const uint8_t *m = p.l2 + 12ull * ((p.flags & kFlagL2One) ? 0ull : i) + 4u * (uint32_t)j;
            g.img0 = (uint32_t)m[0] | ((uint32_t)m[1] << 8) | ((uint32_t)m[2] << 16) | ((uint32_t)m[3] << 24);
        }
        if (j == 3) g.img0 = (g.img0 & 0xffff0000u) | 0x0008u;          // 08 00
        if (j >= 4 && j <= 6) g.img0 &= 0xffff0000u;                     // ip_len, ip_foff, checksum
        if constexpr (TSO) {
            g.hb = o.hlen + g.thl;
            if (g.thl) {   // what every segment gets its own value of leaves the image
                const uint32_t T = 14u + o.hlen, ds = (T + 4u) >> 2, df = (T + 13u) >> 2;
                auto iget = [&](uint32_t d) -> uint32_t {
                    const uint32_t v0 = row_get(g.img0, d & 15u), v1 = row_get(g.img1, d & 15u);
                    return d < 16u ? v0 : v1;
                };
                g.seq0 = __builtin_bswap32((iget(ds) >> 16) | (iget(ds + 1u) << 16));
                g.tfl = iget(df) >> 24;
                g.id0 = swap16(w4 & 0xffffu);
                if (j == 4) g.img0 = 0u;   // ip_id too
                g.img0 &= ~tcp_words((uint32_t)j, T, 0xffffffffu, 0xffu, 0xffffu);
                g.img1 &= ~tcp_words((uint32_t)j + 16u, T, 0xffffffffu, 0xffu, 0xffffu);
            }
        }
        const int hend = 14 + (int)o.hlen;
        const uint32_t k0 = keep_range(g.img0, 4 * j, 14, hend), k1 = keep_range(g.img1, 64 + 4 * j, 14, hend);
        g.hsum = fold64(row_sum((k0 & 0xffffu) + (k0 >> 16) + (k1 & 0xffffu) + (k1 >> 16)));
        if constexpr (L4) {
            const uint32_t m0 = keep_range(g.img0, 4 * j, 0, 14);
            g.mac = fold64(row_sum((m0 & 0xffffu) + (m0 >> 16)));
            g.fidx = o.cnt - 1u;
            if (fo) {
                // the address words as they lie: frame bytes 26..33 (ones::l4_start has the quirks)
                const uint32_t d6 = row_get(g.img0, 6u), d7 = row_get(g.img0, 7u), d8 = row_get(g.img0, 8u);
                uint32_t none = 0u;
                const bool sum = (l4bits & kL4CsumSet) != 0u;
                const uint32_t ps = ones::l4_start(g.proto, __builtin_amdgcn_alignbyte(d7, d6, 2u),
                                                   __builtin_amdgcn_alignbyte(d8, d7, 2u), D - o.hlen, 1u, 0u, none);
                g.ps = sum ? ps : 0u;
                const uint32_t q0 = 14u + o.hlen + fo, dw = q0 >> 2;   // the field in the image: 36..90, even
                const uint32_t v0 = row_get(g.img0, dw & 15u), v1 = row_get(g.img1, dw & 15u);
                const uint32_t wd = dw < 16u ? v0 : v1;
                g.old = (q0 & 2u) ? wd >> 16 : wd & 0xffffu;
                g.fidx = o.max ? fo / o.max : 0u;
                g.qf = q0 - g.fidx * o.max;
                if constexpr (TSO) {
                    if (g.thl) {   // every frame holds the field, at q0; the frame's length joins per frame
                        const uint32_t src = __builtin_amdgcn_alignbyte(d7, d6, 2u), dst = __builtin_amdgcn_alignbyte(d8, d7, 2u);
                        g.ps = 0xffffu + (src & 0xffffu) + (src >> 16) + (dst & 0xffffu) + (dst >> 16) + 0x0600u;
                        g.fidx = o.cnt - 1u;   // in order
                        g.qf = q0;
                    }
                }
            }
        }
        return g;
    };

    // L4: the fragment a row walks as the datagram's frame number t: the one with the field last.
    auto frag_at = [&](const Dg &g, uint32_t t) -> uint32_t {
        if constexpr (L4) return t + 1u == g.cnt ? g.fidx : t + (t >= g.fidx ? 1u : 0u);
        else return t;
    };

    // The row's next datagram that becomes frames; rows with `go` only.
    auto advance = [&](Pos &n, bool go) {
        while (__any(go)) {
            run.take(go && run.cur >= run.end, p.ctr, p.n);
            if (go) {
                if (run.cur >= p.n) {
                    n.act = false;
                    if constexpr (L4) n.pre = false;
                    n.k = 0;
                    n.fr = idle_frame<M>();
                    go = false;
                } else {
                    const Dg g = load_dg(run.cur++);
                    if (g.cnt) {
                        n.g = g;
                        n.jf = 0;
                        n.k = 0;
                        n.act = true;
                        if constexpr (L4) {
                            n.t = 0;
                            n.jf = frag_at(g, 0u);
                            n.fr = frame_of(g, n.jf);
                            n.pre = (g.cnt == 1u || seg_of(g)) && g.qf != 0u && n.fr.m > 1u;
                        } else {
                            n.fr = frame_of(g, 0u);
                        }
                        go = false;
                    }
                }
            }
        }
    };

    auto next = [&](const Pos &c) -> Pos {
        Pos n = c;
        bool adv = false;
        if (c.act) {
            n.k = c.k + 1u;
            if (n.k >= c.fr.m) {
                n.k = 0;
                if constexpr (L4) {
                    if (c.pre) {
                        n.pre = false;   // the same frame again, now with the value
                    } else {
                        n.t = c.t + 1u;
                        if (n.t >= c.g.cnt) {
                            adv = true;
                        } else {
                            n.jf = frag_at(n.g, n.t);
                            n.fr = frame_of(n.g, n.jf);
                            n.pre = (n.t + 1u == n.g.cnt || seg_of(n.g)) && n.g.qf != 0u && n.fr.m > 1u;
                        }
                    }
                } else {
                    n.jf = c.jf + 1u;
                    if (n.jf >= c.g.cnt) adv = true;
                    else n.fr = frame_of(n.g, n.jf);
                }
            }
        }
        if (__any(adv)) advance(n, adv);
        return n;
    };

    auto issue = [&](const Pos &c, Chunk &ch) {
        const int rel = rel_of(c, j);
        const uint64_t sa = c.fr.src + (uint64_t)(int64_t)rel, a4 = sa & ~3ull;
        ch.r = (uint32_t)sa & 3u;
#pragma unroll
        for (int q = 0; q < 6; q++) ch.x[q] = u32x4a4{0u, 0u, 0u, 0u};
        ch.x6 = 0u;
        if (c.act && rel > -kChunkBytes) {
            if (a4 >= p.lo4 && a4 + 4 * (kChunkWords + 1) <= p.hi4) {
                fcs::LoadPriority lp;
#pragma unroll
                for (int q = 0; q < 6; q++) ch.x[q] = fcs::gload<u32x4a4>(a4 + 16 * q);
                ch.x6 = fcs::gload<uint32_t>(a4 + 96);
            } else {   // a window across the arena's edge: dword by dword
                uint32_t d[kChunkWords + 1];
#pragma unroll
                for (int q = 0; q <= kChunkWords; q++) {
                    const uint64_t ad = a4 + 4 * q;
                    d[q] = (ad >= p.lo4 && ad + 4 <= p.hi4) ? fcs::gload<uint32_t>(ad) : 0u;
                }
#pragma unroll
                for (int q = 0; q < 6; q++) ch.x[q] = u32x4a4{d[4 * q], d[4 * q + 1], d[4 * q + 2], d[4 * q + 3]};
                ch.x6 = d[kChunkWords];
            }
        }
    };

    // per-frame state, carried over the frame's segments
    uint32_t s = 0;       // CRC register
    uint32_t carry = 0;   // the last word of the previous segment's lane 0 (the bytes in front of lane 15's chunk)
    // L4: this lane's sum of the frame so far, of the datagram's frames before it (each on its frame
    // start's grid), and the row's new ^ old of the datagram's field once the sum is complete
    uint64_t tot = 0, dsum = 0;
    uint32_t dl4 = 0;

    auto process = [&](const Pos &c, const Chunk &ch) {
        const Frame &fr = c.fr;
        const int rel = rel_of(c, j);
        bool live = c.act;   // a frame that is built, not only summed
        if constexpr (L4) live = c.act && !c.pre;
        const bool first = c.k == 0, last = live && c.k + 1u == fr.m;
        uint32_t d[kChunkWords + 1], w[kChunkWords];   // word i: frame positions rel + 4 i ..
        rxv::unpack(ch.x, ch.x6, d);
        rxv::align_words(d, ch.r, w);
        // ---- the 14 + hlen bytes in front: from the header image (a first segment shorter than
        //      that leaves the rest of them to the second) ----
        const int hend = 14 + (int)hb_of(c.g);
        if (__any(c.act && rel < hend && rel > -kChunkBytes)) {
#pragma unroll
            for (int i = 0; i < kChunkWords; i++) {
                const int q = rel + 4 * i;
                const bool hit = c.act && q > -4 && q < hend;
                if (__any(hit)) {
                    const int D0 = q >> 2, D1 = D0 + 1;   // -1 where the word starts in front of the frame: masked below
                    uint32_t lo = row_get(fr.f0, (uint32_t)D0 & 15u), hi = row_get(fr.f0, (uint32_t)D1 & 15u);
                    if (__any(hit && D1 >= 16)) {
                        uint32_t i1 = c.g.img1;
                        if constexpr (TSO) i1 = fr.f1;
                        const uint32_t lo1 = row_get(i1, (uint32_t)D0 & 15u), hi1 = row_get(i1, (uint32_t)D1 & 15u);
                        lo = D0 >= 16 ? lo1 : lo;
                        hi = D1 >= 16 ? hi1 : hi;
                    }
                    const uint32_t hv = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)q & 3u);
                    const uint32_t pm = fcs::clear_low_bits(0xFFFFFFFFu, 8 * (hend - q));   // bytes from hend on: payload
                    if (hit) w[i] = (w[i] & pm) | (hv & ~pm);
                }
            }
        }
        // ---- padding (rule 8): positions from 14 + I on are zero ----
        if (__any(c.act && fr.I < 56u)) {
            const int pe = 14 + (int)fr.I;
#pragma unroll
            for (int i = 0; i < kChunkWords; i++) w[i] ^= fcs::clear_low_bits(w[i], 8 * (pe - (rel + 4 * i)));
        }
        // ---- the front mask: positions in front of the frame ----
        if (first) {
#pragma unroll
            for (int i = 0; i < kChunkWords; i++) w[i] = fcs::clear_low_bits(w[i], -8 * (rel + 4 * i));
        }
        // ---- L4: the sums, and at the datagram's last frame the field ----
        if constexpr (L4) {
            const bool fend = c.act && c.k + 1u == fr.m;
            const bool seg = seg_of(c.g);                                      // TSO: every frame holds its own field
            const bool fin = c.act && (c.t + 1u == c.g.cnt || seg) && c.g.qf != 0u;   // the frame that holds the field
            const bool again = fin && !c.pre && fr.m > 1u;                    // summed by the visit before
            uint64_t a = 0, b = 0;
            rxv::add_sums(w, rel, 0, 0u, a, b);
            if (first) tot = 0;
            if (c.act && c.g.ps != 0u && !again) tot += a;
            if (__any(fend)) {
                const uint32_t ft = fold64(tot);
                if (fend) dsum += (fr.F & 1u) ? swap16(ft) : ft;   // the end's grid to the start's
                if (__any(fend && fin && !again)) {
                    const rxv::Sums q = rxv::reduce_sums(dsum, 0ull, 0u, false, false);
                    uint64_t x = (uint64_t)c.g.ps + q.tot_s + (uint64_t)c.g.cnt * (0xffffu - c.g.mac) + (0xffffu - c.g.old);
                    if constexpr (TSO) {   // one frame's sum, the pseudo header with this segment's thl + plen
                        const uint64_t xs = (uint64_t)c.g.ps + swap16(fr.I - c.g.hlen) + q.tot_s + (0xffffu - c.g.mac);
                        x = seg ? xs : x;
                    }
                    uint32_t v = c.g.ps ? ~fold64(x) & 0xffffu : 0u;   // TXD_F_UDP_ZERO: 0, nothing summed
                    if (v == 0u && c.g.ps != 0u && c.g.proto == 17u) v = 0xffffu;   // RFC 768
                    if (fend && fin && !again) dl4 = v ^ c.g.old;
                }
                if (fend && ((!c.pre && c.t + 1u == c.g.cnt) || seg)) dsum = 0;   // the datagram (TSO: the frame) is done
            }
            const bool pat = fin && !c.pre;
            if (__any(pat)) xor_field(w, pat ? (int)c.g.qf - rel : rxv::kNoField, dl4);
        }
        // ---- CRC over the words as they will be stored ----
        uint32_t crc = 0u;
        if (FCSW) {
            s = rxv::crc_step(lds, s, w, first, -rel, tb0, tb1);
            if (__any(last)) crc = ~rxv::crc_join(lds, s, last, lanebase);
        }
        // ---- stores, on the destination's dword grid ----
        const uint64_t da = fr.fo + (uint64_t)(int64_t)rel;
        const uint32_t rd = (uint32_t)da & 3u;
        const uint64_t A0 = da - rd;
        const uint32_t up = row_get(w[kChunkWords - 1], (uint32_t)(j + 1) & 15u);
        const uint32_t prevw = j == kGroup - 1 ? carry : up;
        carry = row_get(w[kChunkWords - 1], 0u);
        uint32_t dst[kChunkWords];   // dword t: chunk bytes [4 t - rd, 4 t - rd + 4)
#pragma unroll
        for (int t = 0; t < kChunkWords; t++) {
            const uint32_t al = __builtin_amdgcn_alignbyte(w[t], t ? w[t - 1] : prevw, 4u - rd);
            dst[t] = rd ? al : w[t];
        }
        if (live) {
#pragma unroll
            for (int q = 0; q < 6; q++) {
                const uint64_t ad = A0 + 16 * q;
                if (ad >= fr.fo) {
                    gstore<u32x4a4>(ad, u32x4a4{dst[4 * q], dst[4 * q + 1], dst[4 * q + 2], dst[4 * q + 3]});
                } else if (ad + 16 > fr.fo) {   // the frame's first dwords
#pragma unroll
                    for (int e = 0; e < 4; e++)
                        if (ad + 4 * e >= fr.fo) gstore<uint32_t>(ad + 4 * e, dst[4 * q + e]);
                }
            }
        }
        // the frame's first partial dword: MAC bytes, by byte stores
        if (__any(live && first)) {
            const uint32_t mac0 = row_get(fr.f0, 0u);
            const uint32_t nb = (4u - ((uint32_t)fr.fo & 3u)) & 3u;
            if (live && first && (uint32_t)j < nb) gstore<uint8_t>(fr.fo + (uint32_t)j, (uint8_t)(mac0 >> (8 * j)));
        }
        // the frame's last partial dword and the FCS, by byte stores; flen and fcs of its slot
        if (__any(last)) {
            uint64_t tv = rd ? (uint64_t)(carry >> (8u * (4u - rd))) : 0ull;
            tv |= (uint64_t)crc << (8u * rd);
            const uint32_t nbt = rd + (FCSW ? 4u : 0u);
            if (last && (uint32_t)j < nbt) gstore<uint8_t>(fr.fo + fr.F - rd + (uint32_t)j, (uint8_t)(tv >> (8 * j)));
            const uint64_t slotk = c.g.slot0 + c.jf;
            if (last && j == 15 && p.flen != nullptr) p.flen[slotk] = fr.F;
            if (last && j == 14 && p.fcs != nullptr) p.fcs[slotk] = crc;
        }
    };

    Pos A;
    A.jf = A.k = 0;
    A.act = false;
    if constexpr (L4) {
        A.t = 0;
        A.pre = false;
    }
    A.g = Dg{};
    A.fr = idle_frame<M>();
    advance(A, true);
    rxv::two_in_flight<Chunk>(A, next, issue, process);
}

template <bool FCSW, int NT>
__global__ __launch_bounds__(NT, 1) void txf_kernel(FParams p) {
    frame_walk<FCSW, Mode::kPlain, NT>(p);
}

// ip_tx_frame_l4_*: the framer that also fills every datagram's L4 checksum.
template <bool FCSW, int NT>
__global__ __launch_bounds__(NT, 1) void txd_kernel(FParams p) {
    frame_walk<FCSW, Mode::kL4, NT>(p);
}

// ip_tx_tso_*: that, with eligible TCP datagrams cut into MSS segments.
template <bool FCSW, int NT>
__global__ __launch_bounds__(NT, 1) void tso_kernel(FParams p) {
    frame_walk<FCSW, Mode::kTso, NT>(p);
}

// ---------------------------------------------------------------------------------------------
// The plan: status words and the exclusive prefix sums of the frame counts.
// ---------------------------------------------------------------------------------------------
// first[i] = the frame count of datagram i; tot[block] = the block's sum.
__global__ __launch_bounds__(kPlanThreads) void txf_plan_kernel(FParams p, uint32_t *status, uint64_t *first,
                                                                uint64_t *tot) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    uint64_t cnt = 0;
    if (i < p.n) {
        const uint64_t a = p.dg + p.off[i], a4 = a & ~3ull;
        const uint32_t D = p.len[i], r = (uint32_t)a & 3u;
        uint32_t e[3] = {0u, 0u, 0u};
        if (D >= 20u) {
#pragma unroll
            for (int q = 0; q < 3; q++) {
                const uint64_t ad = a4 + 4 * q;
                if (ad >= p.lo4 && ad + 4 <= p.hi4) e[q] = fcs::gload<uint32_t>(ad);
            }
        }
        const uint32_t w0 = __builtin_amdgcn_alignbyte(e[1], e[0], r), w4 = __builtin_amdgcn_alignbyte(e[2], e[1], r);
        const One o = plan_fields(D, w0 & 0xffu, swap16(w0 >> 16), swap16(w4 >> 16), p.mtu, p.flags);
        if (status != nullptr) status[i] = o.status;
        first[i] = o.cnt;
        cnt = o.cnt;
    }
    uint64_t total;
    plan::block_scan_incl(cnt, sh, total);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// The same for include/nstack_tso.h: header bytes 0..9 and, for candidates (tso_plan.hpp), segment
// bytes 12 and 13; status[i] is the whole word. Every read lies inside the datagram and [lo4, hi4).
__global__ __launch_bounds__(kPlanThreads) void tso_plan_kernel(FParams p, uint32_t *status, uint64_t *first,
                                                                uint64_t *tot) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    uint64_t cnt = 0;
    if (i < p.n) {
        const uint64_t a = p.dg + p.off[i];
        const uint32_t D = p.len[i];
        auto word = [&](uint64_t b) -> uint32_t {   // the four bytes from datagram byte b on (inside the datagram)
            const uint64_t ad = a + b, a4 = ad & ~3ull;
            uint32_t lo = 0u, hi = 0u;
            if (a4 >= p.lo4 && a4 + 4 <= p.hi4) lo = fcs::gload<uint32_t>(a4);
            if ((ad & 3ull) && a4 + 8 <= p.hi4) hi = fcs::gload<uint32_t>(a4 + 4);
            return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)ad & 3u);
        };
        TsoOne t{plan_fields(D, 0u, 0u, 0u, p.mtu, p.flags & kKnownFlags), 0u, 0u};
        if (D >= 20u) {
            const uint32_t w0 = word(0), w4 = word(4), w8 = word(8);
            const uint32_t hlen = (w0 & 0x0fu) * 4u, foff = swap16(w4 >> 16), proto = (w8 >> 8) & 0xffu;
            uint32_t tw = 0u;
            if (hlen >= 20u && hlen <= D && tso_candidate(D, hlen, proto, foff)) tw = word(hlen + 12u);
            uint32_t mss = 0u;
            if (p.mss != nullptr) mss = p.mss[(p.flags & kFlagMssOne) ? 0ull : i];
            t = tso_fields(D, w0 & 0xffu, swap16(w0 >> 16), foff, proto, tw & 0xffu, (tw >> 8) & 0xffu, mss, p.mtu, p.flags);
        }
        if (status != nullptr) status[i] = t.o.status;
        first[i] = t.o.cnt;
        cnt = t.o.cnt;
    }
    uint64_t total;
    plan::block_scan_incl(cnt, sh, total);
    if (threadIdx.x == 0) tot[blockIdx.x] = total;
}

// One workgroup: tot[b] becomes the sum of the blocks in front of b; *total the sum of all.
__global__ __launch_bounds__(kPlanThreads) void txf_scan_totals_kernel(uint64_t *tot, uint64_t nb, uint64_t *total) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t base = plan::scan_totals(tot, nb, sh);
    if (threadIdx.x == 0) *total = base;
}

// first[i] = tot[block] + the counts in front of i within the block.
__global__ __launch_bounds__(kPlanThreads) void txf_add_kernel(uint64_t *first, const uint64_t *tot, uint64_t n) {
    __shared__ uint64_t sh[kPlanThreads];
    const uint64_t i = (uint64_t)blockIdx.x * kPlanThreads + threadIdx.x;
    const uint64_t v = i < n ? first[i] : 0ull;
    const uint64_t excl = plan::block_scan_excl(v, sh);
    if (i < n) first[i] = tot[blockIdx.x] + excl;
}

namespace {
std::atomic<int> g_last_route{(int)Route::kNone}, g_last_route_l4{(int)Route::kNone}, g_last_route_tso{(int)Route::kNone};
}
Route last_launch() { return (Route)g_last_route.load(std::memory_order_relaxed); }
Route last_launch_l4() { return (Route)g_last_route_l4.load(std::memory_order_relaxed); }
Route last_launch_tso() { return (Route)g_last_route_tso.load(std::memory_order_relaxed); }

hipError_t launch_txf(const FParams &p, Mode mode, int cus, hipStream_t st) {
    (void)hipGetLastError();   // report this launch's own error, not an earlier call's
    if (!p.n) return hipSuccess;
    if (!p.ctr) return hipErrorInvalidValue;
    const bool fcsw = (p.flags & kFlagFcs) != 0;
    if (mode == Mode::kTso) g_last_route_tso.store((int)(fcsw ? Route::kTsoFcs : Route::kTso), std::memory_order_relaxed);
    else if (mode == Mode::kL4) g_last_route_l4.store((int)(fcsw ? Route::kGeneralL4Fcs : Route::kGeneralL4), std::memory_order_relaxed);
    else g_last_route.store((int)(fcsw ? Route::kGeneralFcs : Route::kGeneral), std::memory_order_relaxed);
    // one workgroup per CU, persistent over the datagrams (a quarter-wave per run of datagrams)
    const uint64_t rows = kThreads / kGroup, want = (p.n + rows * kRun - 1) / (rows * kRun);
    const int grid = (int)(want < (uint64_t)cus ? want : (uint64_t)cus);
    if (mode == Mode::kTso && fcsw) hipLaunchKernelGGL((tso_kernel<true, kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    else if (mode == Mode::kTso) hipLaunchKernelGGL((tso_kernel<false, kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    else if (mode == Mode::kL4 && fcsw) hipLaunchKernelGGL((txd_kernel<true, kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    else if (mode == Mode::kL4) hipLaunchKernelGGL((txd_kernel<false, kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    else if (fcsw) hipLaunchKernelGGL((txf_kernel<true, kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    else hipLaunchKernelGGL((txf_kernel<false, kThreads>), dim3(grid), dim3(kThreads), 0, st, p);
    return hipGetLastError();
}

namespace {
template <class K>
hipError_t launch_plan_with(K count_kernel, const FParams &p, uint32_t *status, uint64_t *first, uint64_t *tot, hipStream_t st) {
    (void)hipGetLastError();
    if (!p.n) return hipSuccess;
    const uint64_t nb = plan::plan_blocks(p.n);
    if (nb > 0x7fffffffull) return hipErrorInvalidValue;
    PLAN_LAUNCH(count_kernel, dim3((unsigned)nb), dim3(kPlanThreads), 0, st, p, status, first, tot);
    PLAN_LAUNCH(txf_scan_totals_kernel, dim3(1), dim3(kPlanThreads), 0, st, tot, nb, first + p.n);
    PLAN_LAUNCH(txf_add_kernel, dim3((unsigned)nb), dim3(kPlanThreads), 0, st, first, (const uint64_t *)tot, p.n);
    return hipSuccess;
}
}  // namespace

hipError_t launch_plan(const FParams &p, uint32_t *status, uint64_t *first, uint64_t *tot, hipStream_t st) {
    return launch_plan_with(txf_plan_kernel, p, status, first, tot, st);
}

hipError_t launch_plan_tso(const FParams &p, uint32_t *status, uint64_t *first, uint64_t *tot, hipStream_t st) {
    return launch_plan_with(tso_plan_kernel, p, status, first, tot, st);
}

}  // namespace txf
