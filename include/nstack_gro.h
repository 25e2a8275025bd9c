/*
 * nstack_gro.h — C ABI of one-pass RX coalescing (same library, libnstack_fcs.so).
 *
 * nstack_tso.h cuts a large TCP send into MSS-sized segments; nstack_rxr.h and nstack_rxd.h undo IP
 * fragmentation but hand every one of those segments to the caller's tcp_input as a datagram of its
 * own. These calls are the inverse of nstack_tso.h, the step a NIC's LRO or a kernel's GRO does: runs
 * of in-order, header-compatible TCP segments of one flow leave as one large TCP datagram. The
 * reference has no such step, so this is NEW BEHAVIOUR throughout and OPT-IN: nstack's sources stay
 * untouched, and ether_rx_reasm_* and ip_rx_reasm_l4_* keep their bytes, status words, launch names
 * and symbols. Its tcp_input checks one checksum per datagram handed to it (src/tcp.c:508-515, as
 * nstack_rxd.h cites), so a merged datagram carries a valid one.
 *
 * Everything that is not coalesced comes out as ether_rx_reasm_plan_* plus ip_rx_reasm_l4_* give it,
 * byte for byte and word for word (but for GRO_CAND in the status word): a mixed batch is one call.
 *
 * The frames, F, T, P, I, hlen and the plan arrays are those of nstack_rxr.h. seg is the datagram from
 * byte hlen on.
 *
 * Rules for frame i (status word bits in capitals):
 *   1. Rules 1-5 of nstack_rxr.h hold first, with the same status bits. Fragments are grouped,
 *      reassembled and placed by its rules 6-7, unchanged. A reassembled datagram is never a candidate.
 *   2. GRO_CAND        an RXR_WHOLE frame with all of: ip_proto == 6; L = I - hlen >= 20;
 *                      thl = (seg[12] >> 4) * 4 with 20 <= thl <= L; P = L - thl >= 1 (a pure ACK is
 *                      no candidate); (seg[13] & (SYN | RST | URG)) == 0; I <= 32768 (a design limit:
 *                      rule 4 has the reason).
 *      The flow key is ip_src, ip_dst, source port and destination port as the bytes lie.
 *      seq = ntohl(seg[4..8)). The group key is (flow, seq >> 15): a group is the candidates of one
 *      flow whose first byte lies in one 32 KiB window of ABSOLUTE sequence space. The cut points
 *      depend on the segments alone, never on what else is in the batch; 2^32 is a multiple of the
 *      window, so no group wraps.
 *   3. A group of two or more members is coalescible when all of these hold:
 *      (a) no two members have the same seq;
 *      (b) exactly one member's end (seq + P) mod 2^32 is not the seq of another member of the group;
 *          that member is the last one;
 *      (c) the sum of P equals the last member's end minus the lowest seq;
 *      (d) every member has the first member's hlen and thl, and agrees with it in every IP header
 *          byte but 2-3, 4-5 and 10-11, and in every TCP header byte but 4-7, the FIN / PSH / CWR
 *          bits of byte 13, and 16-17: TOS, TTL, DF, IP options, ACK number, window and TCP options
 *          must match. DEVIATION from Linux GRO: ip_id is not compared (nstack_tso.h writes
 *          counting or fixed ids, and a receiver cannot know which);
 *      (e) FIN or PSH is set on no member but the last, and CWR on no member but the first.
 *      By (a) the member with the lowest seq, the first, is unique. (a)-(c) together mean the members
 *      tile one range with no gap, overlap or duplicate, by the argument of nstack_rxr.h rule 6: every
 *      member but the last has a successor that starts at its end, and P >= 1, so seq only goes
 *      upward along the successor chain from any member; the chain cannot cycle inside a window and
 *      ends at the one member without a successor. The chain from the first member covers
 *      [lowest seq, last end) exactly once; a member outside that chain would make the sum exceed
 *      the range.
 *      Otherwise every member stays what it was: an RXR_WHOLE datagram of its own, with GRO_CAND
 *      set. A dropped frame (rule 1) is no member, so a loss, a retransmitted duplicate or a bad
 *      checksum in a window leaves that window unmerged. There is no carried state, as in reassembly.
 *   4. Merged datagram. GRO_MERGED on every member; the first also carries RXR_HEAD, plus GRO_FIN /
 *      GRO_PSH when the last member has that flag. Its bytes are the first member's hlen + thl header
 *      bytes, then the payload of member x at hlen + thl + (seq_x - seq_first).
 *      D = hlen + thl + sum of P. The sum is at most 32767 + P_last and the header lengths are equal,
 *      so D <= 32767 + I_last <= 65535: that is what the I <= 32768 limit buys.
 *      Patched fields: ip_len = htons(D); the IP header checksum recomputed and stored as
 *      nstack_rxr.h rule 7 stores it; ip_foff is kept as it lies, so DF survives; the TCP flags byte
 *      is first | (last & (FIN | PSH)); the TCP checksum is tcp_checksum over the D - hlen delivered
 *      bytes with that length in the pseudo header, stored as nstack_txs.h rule 6 stores it. Every
 *      other byte is the first member's.
 *      The members' own checksums are NOT checked here: the caller drops bad frames with the
 *      validator's verdicts and drop_mask (rule 1), and a frame it does not drop is merged as it is.
 *   5. Order and placement follow nstack_rxr.h rule 8. A merged datagram's head frame is its first
 *      member (lowest seq, not lowest index). RXR_NO_ROOM and RXR_DELIVERED mean what they mean there.
 *   6. Datagram verdict word: a merged datagram gets GROD_MERGED | 6 << RXD_PROTO_SHIFT; every other
 *      datagram gets nstack_rxd.h rules 1-3 word for word, so a lone segment still has its checksum
 *      judged.
 *   7. The result is a function of the input alone, never of scheduling.
 *
 * The device plan is ether_rx_reasm_plan_dev's seven launches with five more between them (candidate
 * records, insert, link, first-member compare in front of the decide launch; the members' places
 * behind the finish launch), behind two memsets, with at most 224 bytes of scratch per frame from
 * hipMallocAsync: the 96 of nstack_rxr.h, a 32-byte segment record, a 32-byte group accumulator
 * (lowest seq, highest end, sum of P, members without a successor, fault flag, member count, the
 * last's flags) and two open-addressing tables of 8-byte entries with at least two and fewer than
 * four entries per frame each, keyed by (flow, seq) with an arrival count and by (flow, seq >> 15).
 * No workgroup waits for another; data passes between the phases only across kernel boundaries; every
 * probe loop is bounded by the table size, and the tables cannot fill. The first member is found by
 * looking up (flow, lowest seq) in a launch after the one that settled the minimum.
 * The build is nstack_rxd.h's summing build with a skip of hlen + thl on members behind the first and
 * the head patch of rule 4; the finishing launch (one thread per datagram, across a kernel boundary)
 * reads a merged datagram's header back, takes the IP header and the old checksum field out of the
 * sum, adds the pseudo header, and stores the TCP checksum and the verdict word. The guards of
 * ether_rx_reasm_dev hold for any plan arrays; verdict words of a plan no plan call wrote are
 * unspecified.
 *
 * Errors, the -ENODEV behaviour without a usable gfx950 GPU (no CPU path), thread safety and the
 * untouched host-fallback counters are those of nstack_rxd.h.
 */
#ifndef NSTACK_GRO_H
#define NSTACK_GRO_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status bits, next to those of nstack_rxr.h */
#define GRO_CAND     0x1000u   /* rule 2 */
#define GRO_MERGED   0x2000u   /* a member of a merged datagram; with RXR_HEAD: its first member */
#define GRO_FIN      0x4000u   /* on the first member: the last member has FIN */
#define GRO_PSH      0x8000u   /* on the first member: the last member has PSH */

/* datagram verdict bit, next to those of nstack_rxd.h */
#define GROD_MERGED  0x400u

/* Host arithmetic, no GPU: ether_rx_reasm_plan_host's arguments and errors. Returns m. It sizes `out`
 * (doff[m]) and is the plan the host form uses. */
int64_t ip_rx_gro_plan_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                            uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat,
                            uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead);

/* Device plan: ether_rx_reasm_plan_dev's arguments; the same arrays, and counts. */
int ip_rx_gro_plan_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, uint32_t *fstat,
                       uint64_t *dst, uint32_t *dgi, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint64_t *counts,
                       void *stream);

/* Device build plus finishing launch: ip_rx_reasm_l4_dev's arguments, on arrays ip_rx_gro_plan_dev left. */
int ip_rx_gro_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n, uint32_t flags,
                  const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi, const uint64_t *doff, const uint32_t *dlen,
                  const uint64_t *counts, void *out, uint64_t out_bytes, uint32_t *fstat, uint32_t bad_mask,
                  uint32_t *dverdict, uint64_t *bad, void *stream);

/* Host batch: ip_rx_reasm_l4_host's arguments; its chunks are reported by fcs_debug_rxr_last_host_chunks. */
int64_t ip_rx_gro_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align, void *out,
                       uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen, uint32_t *dlead, uint32_t bad_mask,
                       uint32_t *dverdict, uint64_t *bad);

/* Introspection for the tests: the kernel the last coalescing build launch of this process took
 * ("gro", "none"). Returns the name's length or -EINVAL. */
int fcs_debug_gro_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_GRO_H */
