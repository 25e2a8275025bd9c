/*
 * nstack_txf.h — C ABI of one-pass TX framing (same library, libnstack_fcs.so).
 *
 * Framing turns IPv4 datagrams into wire-ready Ethernet frames: what the reference does on the host
 * in ip_send_fragments (src/ip.c:225-269: cut the payload, rewrite ip_len and ip_foff, recompute the
 * header checksum through ip_hton, ip.c:79-80) and in ether_send (src/linux/ether.c:222-263: the
 * 14-byte header in front, zero padding, the FCS behind). One launch reads every payload byte of a
 * batch once and writes it once. It closes the transmit path in front of nstack_txs.h (which
 * finishes frames that exist) and is the producer of what nstack_rxv.h checks. An OPT-IN entry
 * point: nstack's sources stay untouched.
 *
 * Datagram i is D = len[i] bytes at dgram + off[i]: an IPv4 header of hlen = (vhl & 0x0f) * 4 bytes
 * and B = D - hlen payload bytes, in network byte order as ip_hton leaves it. mtu is a call
 * argument, 76 <= mtu <= 65535, so that the fragment payload unit of rule 6 is at least 8 for every
 * hlen. The output arena must not overlap the datagrams.
 *
 * Rules for datagram i (status word bits in capitals):
 *   1. TXF_BAD_HDR     D < 20, or (vhl & 0x40) != 0x40 (src/ip.c:130, quirk kept), or hlen < 20, or
 *                      hlen > D. No frames. The later rules are not evaluated.
 *   2. TXF_BAD_LEN     ntohs(ip_len) != D (ip.c:141, ip.c:318). No frames; rules 3-6 are not evaluated.
 *   3. TXF_WHOLE       D <= mtu: one frame carries the datagram as it is; the ip_foff bytes are
 *                      kept and only the header checksum is rewritten (rule 7).
 *                      DEVIATION: ip.c:326 compares the payload size with ETHER_DATA_LEN, so the
 *                      reference hands datagrams of 1501..1520 bytes to ether_send, which refuses
 *                      them (ether.c:234-236). Here those datagrams are fragmented.
 *   4. TXF_REFRAG      D > mtu and ntohs(ip_foff) & 0x3fff non-zero: the input is itself a
 *                      fragment. No frames: the reference would overwrite the offset (ip.c:256);
 *                      re-fragmenting is out of scope.
 *   5. TXF_DF_DROP     D > mtu, TXF_F_HONOR_DF given and ntohs(ip_foff) & 0x4000 set. No frames.
 *                      Without the flag the datagram is fragmented regardless, as ip.c:329 does.
 *                      Independent of rule 4: both bits can be set.
 *   6. TXF_FRAGMENTED  D > mtu and no rule above stopped the datagram. The payload unit is
 *                      max = (mtu - hlen - 8 + 7) & ~7 (ip.c:220-233, the 8-byte shortfall kept:
 *                      1472 at mtu 1500 and hlen 20, so full fragments are 1506-byte frames, not
 *                      1514). cnt = ceil(B / max) fragments (cnt <= 8185; every offset fits 13 bits).
 *                      Fragment j carries payload bytes [j*max, j*max + plen_j), plen_j =
 *                      min(max, B - j*max), behind the datagram's whole hlen header bytes (options
 *                      go into every fragment, as the reference leaves them in place), with
 *                      ip_len = htons(hlen + plen_j) and
 *                      ip_foff = htons((j < cnt - 1 ? 0x2000 : 0) | (j*max >> 3)): the DF and
 *                      reserved bits are cleared, as ip.c:256 does.
 *   7. IP checksum of every frame: ip_checksum(header with bytes 10, 11 zero, hlen), stored as
 *      nstack_txs.h rule 3 stores it (ip.c:79-80: the uint16_t as it is, no byte swap).
 *   8. Frame build (ether.c:222-263): dst[6] src[6] 08 00, the I = hlen + plen IP bytes (I = D for a
 *      TXF_WHOLE frame), zero bytes up to 56 payload bytes: F = 14 + max(I, 56), so the shortest
 *      frame is 70 bytes (ETHER_MINLEN - ETHER_FCS_LEN, quirk kept). With TXF_F_FCS the four bytes
 *      [F, F + 4) hold ether_fcs over the F bytes, little-endian (ether.c:262-263). The MAC pair
 *      comes from l2[i]; with TXF_F_L2_ONE from l2[0] for the whole batch.
 *   9. Placement: frame slot k is out + k * slot, k < slots; slot >= max(14 + mtu, 70) (+ 4 with
 *      TXF_F_FCS), else -EINVAL. Datagram i owns slots [first[i], first[i] + cnt_i); flen[k] = F.
 *      TXF_NO_ROOM: the datagram's slots do not lie inside [0, slots); none of its frames is
 *      written. No byte of `out` other than the F (+ 4) bytes of produced frames is written: the
 *      rest of each slot, and unused slots, keep their content. No byte of a datagram outside
 *      [off[i], off[i] + D) is interpreted.
 *  10. L4 checksums are NOT touched. A fragmented datagram's UDP or TCP checksum spans its fragments
 *      and must be in place before framing: use inet_csum_* (nstack_inet.h), or leave 0 for UDP as
 *      src/udp.c:192 effectively does. TXF_WHOLE frames can go through ether_tx_seal_* afterwards.
 *      ip_tx_frame_l4_* (nstack_txd.h) is this build with the L4 checksum of every datagram filled
 *      in the same launch: it removes that extra pass.
 * A produced frame (F + 4 bytes with TXF_F_FCS) passes ether_rx_validate_* with RXV_F_TRAILER with
 * no defect bit other than RXV_FRAG on fragments and RXV_IP_BAD_LEN on padded frames (I < 56).
 *
 * There is no CPU path for frame building, as for nstack_rxv.h and nstack_txs.h: without a usable
 * gfx950 GPU the device and host forms return -ENODEV, and HIP errors are returned (-ENOMEM, -EIO),
 * never answered on the host; the FCS engine's host-batch and fallback counters are not touched.
 * Errors: 0 (host form: the frame count) or -errno; -EINVAL for unknown flag bits and bad geometry
 * (decided before any device call); text in fcs_last_error(). Thread-safe.
 */
#ifndef NSTACK_TXF_H
#define NSTACK_TXF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags */
#define TXF_F_FCS       1u  /* also write the FCS of each frame at [F, F + 4) */
#define TXF_F_HONOR_DF  2u  /* rule 5: a datagram with DF set that does not fit is dropped, not fragmented */
#define TXF_F_L2_ONE    4u  /* l2[0] serves the whole batch */

/* status bits */
#define TXF_WHOLE       0x001u
#define TXF_FRAGMENTED  0x002u
#define TXF_BAD_HDR     0x004u
#define TXF_BAD_LEN     0x008u
#define TXF_REFRAG      0x010u
#define TXF_DF_DROP     0x020u
#define TXF_NO_ROOM     0x040u  /* set next to TXF_WHOLE or TXF_FRAGMENTED; never by the plan call */

/* The Ethernet addresses of a datagram's frames (12 bytes, no alignment needed). */
struct txf_l2 { uint8_t dst[6], src[6]; };

/* Rules 3 and 6 as host arithmetic: the number of frames a datagram of D bytes with an hlen-byte
 * header becomes at this mtu; 0 for arguments rule 1 or the mtu bound refuses. No GPU needed. */
uint32_t ether_tx_frame_count(uint32_t D, uint32_t hlen, uint32_t mtu);

/* ---- device-resident batches: asynchronous on `stream` (a hipStream_t or NULL), on the calling
 *      thread's current device; dgram, off, len (n entries each), l2, first, out, flen, status and
 *      fcs are device memory ---- */
/* Plan: status[i] (n u32, may be NULL) from rules 1-5 and first[0..n] (n + 1 u64): the exclusive
 * prefix sums of the frame counts, first[n] the total. A small kernel reads the first 8 bytes of
 * each header; the scan is reduce, scan of block totals, add, in separate launches. */
int ether_tx_frame_plan_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t mtu, uint32_t flags, uint32_t *status, uint64_t *first,
                            void *stream);
/* Build: first[i] (n entries are read) may come from the plan call or be any array that gives every
 * datagram cnt_i disjoint slots. status (n u32: the rules re-evaluated, plus TXF_NO_ROOM), flen and
 * fcs (one u32 per slot, written for produced frames only; fcs is 0 without TXF_F_FCS) may each be
 * NULL. */
int ether_tx_frame_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, const uint64_t *first,
                       void *out, uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status, uint32_t *fcs,
                       void *stream);

/* ---- host batch (host memory in and out; synchronous): plans on the host, then runs a chunked
 *      H2D -> kernel -> D2H pipeline over datagram ranges on the engine's first GPU and brings back
 *      the frames and flen. Frames are packed: datagram i owns the slots behind those of datagram
 *      i - 1. Every datagram and the slot capacity are checked before any work: -EINVAL names the
 *      first datagram outside the arena, -ENOSPC is returned when `slots` is too small, and nothing
 *      has been written in either case. status and flen may be NULL. Returns the number of frames.
 *      A HIP error in the middle of a batch (-ENOMEM, -EIO) can leave `out` partly written: the chunks
 *      finished before it are in place, status[] is not written; the call can simply be repeated. */
int64_t ether_tx_frame_host(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                            const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, void *out,
                            uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status);

/* Introspection for the tests: the kernel the last frame-building launch of this process took
 * ("general-fcs", "general", "none"). Returns the name's length or -EINVAL. */
int fcs_debug_txf_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_TXF_H */
