/*
 * nstack_rxr.h — C ABI of one-pass RX reassembly (same library, libnstack_fcs.so).
 *
 * Reassembly turns received Ethernet frames back into IPv4 datagrams: what the reference does on
 * the host in ether_receive's payload copy (src/linux/ether.c:180-212), ip_input's header rules
 * (src/ip.c:119-187) and ip_fragment_input (src/ip_fragment.c:140-203). It is the inverse of
 * nstack_txf.h and the consumer of what nstack_rxv.h checks: a plan (a handful of small launches)
 * groups the fragments of a batch, one build launch reads every delivered byte once and writes it
 * once. An OPT-IN entry point: nstack's sources stay untouched.
 *
 * Frame i is F = len[i] bytes at arena + off[i]. T = 4 with RXR_F_TRAILER, else 0. P = F - 14 - T.
 *
 * Rules for frame i (status word bits in capitals):
 *   1. RXR_DROPPED     a verdict array is given and (verdict[i] & drop_mask) != 0 (the words
 *                      ether_rx_validate_* writes). Nothing further is evaluated. Reassembly itself
 *                      computes no CRC and checks no checksum; ip.c:147-155 has its check under "#if 0".
 *   2. RXR_NOT_IPV4    nstack_rxv.h rules 2 and 3: F < 14 + T (runt), or frame bytes 12, 13 are not
 *                      0x0800 (ether.c:204 reports h_proto; the caller hands other types elsewhere). Nothing further.
 *      RXR_BAD_HDR     nstack_rxv.h rule 4: P < 20, or (vhl & 0x40) != 0x40 (ip.c:130, quirk kept),
 *                      or hlen = (vhl & 0x0f) * 4 < 20 (ip.c:136), or hlen > P. Nothing further.
 *   3. RXR_BAD_LEN     I = ntohs(ip_len); I < hlen or I > P. Nothing further.
 *                      DEVIATION from ip.c:141, which wants I == P: padding and trailer behind I are
 *                      stripped, otherwise the framer's own padded frames (nstack_txf.h rule 8) could
 *                      not come back.
 *   4. RXR_WHOLE       (ntohs(ip_foff) & 0x3fff) == 0 (not ip_fragment_is_frag, ip.c:180): the
 *                      datagram is frame bytes [14, 14 + I) unchanged, header checksum included.
 *   5. RXR_FRAG        otherwise (ip.c:180-184 -> ip_fragment_input): L = I - hlen payload bytes belong at
 *                      o = (foff & 0x1fff) * 8 (ip_fragment.c:142); MF = foff & 0x2000.
 *      RXR_FRAG_BAD    L == 0 or o + L + 20 > 65535 (the reference bounds o alone, ip_fragment.c:146; its buffer
 *                      write at ip_fragment.c:155 is unchecked). Such a frame joins no group.
 *      RXR_HEAD        o == 0 (on a fragment that is not RXR_FRAG_BAD).
 *   6. Group key: (ip_src, ip_dst, ip_proto, ip_id) as the bytes lie in the header: packet_buf_cmp's
 *      bufid, ip_fragment.c:39-65. A group is complete exactly when its fragments tile [0, total)
 *      with no gap and no overlap: exactly one head; exactly one fragment without MF, which ends at
 *      total; no two fragments with the same o; every MF fragment's end o + L is the o of another
 *      fragment; and the sum of L equals total. (Offsets only go upward along the successor chain
 *      from 0, which ends at the one fragment without a successor; a fragment outside the chain would
 *      make the sum exceed total.)
 *      RXR_INCOMPLETE  every fragment of a group that is not complete; nothing of it is written.
 *                      Duplicates, overlaps and a key reused by two datagrams in one batch land here.
 *                      DEVIATION: the reference overwrites on overlap (ip_fragment.c:155), holds four
 *                      static buffers (ip_fragment.c:32) and a timer that is never registered. Here
 *                      there is no carried state and no timer: a caller keeps incomplete frames and
 *                      names them again in its next batch (off[] / len[] point anywhere).
 *      RXR_TOO_BIG     the group is complete but hlen_head + total > 65535: every fragment of it
 *                      carries the bit, and nothing of it is written.
 *   7. Reassembled datagram: the head's hlen_head header bytes (options kept; the other fragments'
 *      headers are discarded), followed by the payload bytes at their offsets. Patched header
 *      fields: ip_len = htons(hlen_head + total), ip_foff = 0, and the header checksum recomputed
 *      and stored as nstack_txs.h rule 3 stores it.
 *      DEVIATION: ip_fragment.c:167 leaves the header length out of ip_len.
 *   8. Order and placement: a datagram's head frame is the RXR_WHOLE frame itself or the group's
 *      RXR_HEAD fragment; datagram k is the k-th head frame in frame order among the datagrams that
 *      rules 1-7 deliver. D = dlen[k] is its length, dlead[k] its head frame's index (the caller
 *      finds the Ethernet header there), doff[k] the exclusive prefix sum of
 *      (D + align - 1) & ~(align - 1), doff[m] the byte total; align is a power of two, 1..128.
 *      The result is a function of the input alone, never of scheduling.
 *      RXR_NO_ROOM     doff[k] + D > out_bytes: none of that datagram's bytes is written; every one
 *                      of its frames carries the bit. Set by the build call only.
 *      RXR_DELIVERED   the frame's bytes went out. Set by the build call only.
 *      No byte of `out` outside delivered datagrams is written: alignment gaps keep their content.
 *      No byte outside a frame is interpreted.
 *
 * There is no CPU path for the build, as for nstack_rxv.h, nstack_txs.h and nstack_txf.h: without a
 * usable gfx950 GPU the device and host forms return -ENODEV, and HIP errors are returned (-ENOMEM,
 * -EIO), never answered on the host; the FCS engine's host-batch and fallback counters are not
 * touched. Errors: 0 (plan_host and the host form: the datagram count m) or -errno; -EINVAL for
 * unknown flag bits, an align that is no power of two in 1..128, NULL arrays with n > 0 and
 * n >= 2^30 (decided before any device call); text in fcs_last_error(). Thread-safe.
 */
#ifndef NSTACK_RXR_H
#define NSTACK_RXR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags */
#define RXR_F_TRAILER   1u   /* frames include their 4-byte FCS (as RXV_F_TRAILER): it is stripped */

/* status bits */
#define RXR_WHOLE       0x001u
#define RXR_FRAG        0x002u
#define RXR_HEAD        0x004u
#define RXR_DROPPED     0x008u
#define RXR_NOT_IPV4    0x010u
#define RXR_BAD_HDR     0x020u
#define RXR_BAD_LEN     0x040u
#define RXR_FRAG_BAD    0x080u
#define RXR_INCOMPLETE  0x100u
#define RXR_TOO_BIG     0x200u
#define RXR_NO_ROOM     0x400u   /* never set by the plan calls */
#define RXR_DELIVERED   0x800u   /* never set by the plan calls */

#define RXR_NONE32 0xffffffffu              /* dgi[i] of a frame that belongs to no delivered datagram */
#define RXR_NONE64 0xffffffffffffffffull    /* dst[i] of such a frame */

/* The plan arrays of a batch of n frames:
 *   fstat[n]     u32  rules 1-7
 *   dst[n]       u64  byte offset in `out` of the frame's first delivered byte, else RXR_NONE64
 *   dgi[n]       u32  the frame's datagram index, else RXR_NONE32
 *   doff[n + 1]  u64  doff[0..m] are written
 *   dlen[n]      u32  dlen[0..m) are written
 *   dlead[n]     u32  dlead[0..m) are written; may be NULL
 * verdict may be NULL (no frame is dropped by rule 1). */

/* Host arithmetic, no GPU: frames and plan arrays in host memory. Every frame is checked against the
 * arena first: -EINVAL names the first one outside it and nothing has been written. Returns m. It
 * sizes `out` (doff[m]) and is the plan the host form uses. */
int64_t ether_rx_reasm_plan_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                                 uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask,
                                 uint32_t align, uint32_t *fstat, uint64_t *dst, uint32_t *dgi, uint64_t *doff,
                                 uint32_t *dlen, uint32_t *dlead);

/* ---- device-resident batches: asynchronous on `stream` (a hipStream_t or NULL), on the calling
 *      thread's current device; every array is device memory ---- */
/* Plan: the same arrays, plus counts[2] = {m, doff[m]} (u64, may be NULL). Seven small launches behind
 * one memset on the stream (classify, insert, link, decide with the block totals, the scan of the
 * totals, place, finish) with at
 * most 96 bytes of scratch per frame from hipMallocAsync: a 16-byte key record, a 32-byte group
 * accumulator, a 4-byte head index and an open-addressing table of 8-byte entries with at least two
 * and fewer than four entries per frame, keyed by (key, o). No workgroup waits for another; data
 * passes between the phases only across kernel boundaries; every probe loop is bounded by the table
 * size, and the table cannot fill.
 * A frame that does not lie inside [arena, arena + arena_bytes) is planned as a frame of no bytes: it
 * is RXR_NOT_IPV4 (the runt of rule 2) and nothing of it is read. (The host calls refuse such a batch
 * with -EINVAL instead; a device call cannot return what only a kernel sees.) */
int ether_rx_reasm_plan_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align,
                            uint32_t *fstat, uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen,
                            uint32_t *dlead, uint64_t *counts, void *stream);
/* Build: pstat, dst, dgi, doff and dlen as a plan call left them. Every frame with dst[i] != RXR_NONE64
 * copies its bytes to out + dst[i]; a head fragment also patches the three header fields of rule 7.
 * fstat (n u32: pstat plus RXR_NO_ROOM or RXR_DELIVERED) may be NULL and may be pstat itself. A frame
 * whose plan entries do not fit its own bytes or `out` is treated as RXR_NO_ROOM: nothing outside
 * [out, out + out_bytes) is written and nothing outside the frames is read, whatever the plan says. */
int ether_rx_reasm_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi,
                       const uint64_t *doff, const uint32_t *dlen, void *out, uint64_t out_bytes, uint32_t *fstat,
                       void *stream);

/* ---- host batch (host memory in and out; synchronous): plans with ether_rx_reasm_plan_host, then
 *      runs a chunked H2D -> kernel -> D2H pipeline over datagram ranges on the engine's first GPU:
 *      a chunk is a run of consecutive datagrams with their frames gathered back to back into
 *      staging; the datagrams are copied back one by one, so alignment gaps keep their content.
 *      Every frame and the capacity are checked before any work: -EINVAL names the first frame
 *      outside the arena, -ENOSPC is returned when a datagram would be RXR_NO_ROOM (out_bytes is smaller
 *      than the last datagram's end, doff[m - 1] + dlen[m - 1]), and nothing has been written in either case. fstat (final), doff, dlen and dlead may each be NULL. Returns m.
 *      A HIP error in the middle of a batch can leave `out` partly written; the call can simply be
 *      repeated. */
int64_t ether_rx_reasm_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align,
                            void *out, uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen,
                            uint32_t *dlead);

/* Introspection for the tests: the kernel the last build launch of this process took ("general",
 * "none"). Returns the name's length or -EINVAL. */
int fcs_debug_rxr_last_launch(char *out, uint64_t cap);
/* The chunks the calling thread's last ether_rx_reasm_host cut its batch into: returns their number
 * and writes the number of datagrams of chunk k to dgs[k] for k < cap (dgs may be NULL with cap 0). */
int64_t fcs_debug_rxr_last_host_chunks(uint64_t *dgs, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_RXR_H */
