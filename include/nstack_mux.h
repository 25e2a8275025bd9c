/*
 * nstack_mux.h — C ABI of one-pass TX multiplexing (same library, libnstack_fcs.so).
 *
 * nstack_dmx.h is the last hop of RX: datagrams in, per-socket queues of struct nstack_dgram records
 * out. These calls are its TX inverse, the socket layer's send side: per-socket SEND queues of such
 * records in, finished IPv4 datagrams out, in the arrays ip_tx_frame_l4_dev and ip_tx_tso_dev read
 * (dgram, off[], len[], one struct txf_l2 per datagram). It is the work the reference does per call in
 * nstack_udp_send (src/udp.c:176-206), tcp_send_segments / nstack_tcp_send (src/tcp.c:614-644, :672-)
 * and ip_send (src/ip.c:278-344), which finds the route with ip_route_find_by_network
 * (src/ip_route.c:132-166) and the neighbour's MAC with arp_cache_get_haddr (src/arp.c:122-138), then
 * writes the header template, ip_id = ip_global_id++ and ip_hton. Every payload byte is read once and
 * written once. NEW and OPT-IN: nothing that exists changes a byte, a status word, a launch name or a
 * launch.
 *
 * Inputs. The send queues are socket-major, the layout demux writes: q, q_bytes; rec[n], the u64
 * offsets of the records inside q (struct nstack_dgram on LP64, nstack_dmx.h rule 6: a 24-byte header
 * {u32 src addr, i32 src port, u32 dst addr, i32 dst port, u64 buf_size}, then buf_size payload
 * bytes); sfirst[S + 1], u64, monotone, sfirst[0] = 0, sfirst[S] = n: the records of socket s are the
 * k in [sfirst[s], sfirst[s + 1]), in send order. bind[S], 0 <= S <= 65536, holds the demux keys
 * (proto << 48 | port << 32 | addr, proto 6 or 17): the socket gives the protocol and the SOURCE port,
 * as sock->info.sock_addr.port does in the reference (src/udp.c:189). tcb[S] (may be NULL) is read for
 * TCP sockets only; the reference's values are send_next, recv_next, 502 and PSH | ACK
 * (src/tcp.c:627-628, :715-717).
 *
 * rt[R], 0 <= R <= 256, is struct ip_route with the interface's own MAC in place of the handle. The
 * lookup is ip_route_find_by_network, step for step:
 *     (a) the lowest index with network == dst;
 *     (b) else the lowest index with network == (dst & netmask);
 *     (c) else the lowest index with network == 0.
 * The table order is the caller's: the reference walks its tree in route_network_cmp order
 * (RB_FOREACH, src/ip_route.c:144), and the caller lists the routes in that order. LIMIT: gw is
 * ignored, as the reference ignores it ("TODO GW support", src/ip.c:22): the neighbour looked up is
 * the destination itself.
 * nb[N], 0 <= N <= 65536, is the ARP cache. The match is exact on addr; an address that occurs more
 * than once belongs to its lowest index (valid entries only); an entry with valid == 0 matches
 * nothing, like age < 0 at src/arp.c:127.
 * id0 is the batch's first ip_id. align is a power of two in 4..128: datagram starts are multiples of
 * it inside dgram. The device forms want q aligned to 8, himg to 4 and dgram to align.
 *
 * Rules for record k of socket s (status bits of mstat[k] in capitals).
 *   1. MUX_BAD_REC    rec[k] is no multiple of 8, or rec[k] + 24 > q_bytes, or
 *                     rec[k] + 24 + buf_size > q_bytes; or the record's destination port lies outside
 *                     0..65535; or the socket's key is invalid (proto neither 6 nor 17, or bits 56..63
 *                     set). In the device forms also: no socket's range holds k (an sfirst that is
 *                     not what this header asks for). Nothing else is looked at.
 *   2. MUX_BAD_SIZE   P = buf_size. UDP: unless 0 < P < 65507 (src/udp.c:182, the strict bound kept).
 *                     TCP: P > 65495. P = 0 is built on TCP: a bare segment with the tcb's flags.
 *      MUX_NO_TCB     a TCP socket with tcb == NULL. Both bits may be set; either ends the rules.
 *   3. MUX_NO_ROUTE   no route for the record's dstaddr.inet4_addr (src/ip.c:284-291).
 *   4. MUX_NO_NEIGH   the route was found and the neighbour was not. The reference defers the
 *                     datagram and sends an ARP request (src/ip.c:293-310). DEVIATION: here the record
 *                     keeps its status word and makes no datagram; deferral and ARP stay with the
 *                     caller.
 *   5. MUX_PLANNED    the record passed rules 1-4. Its datagram is hl + P bytes: 20 of IP header, then
 *                     8 of UDP or 20 of TCP (hl = 28 or 40).
 *        IP   45 00, ip_len, ip_id, 40 00 (IP_TOFF_DEFAULT), ttl 64, proto, checksum, ip_src, ip_dst.
 *             ip_src is the route's iface (src/ip.c:320), not the record's srcaddr, which the
 *             reference does not use for the header either. ip_id = (id0 + r) & 0xffff, r the number
 *             of MUX_PLANNED records with a lower k: the ids ip_global_id++ would hand out if the
 *             records were sent in order. The header checksum is what ip_hton stores
 *             (src/ip.c:79-80; stored as nstack_txs.h rule 3 stores it): the datagram is valid on its
 *             own.
 *        UDP  sport, dport, udp_len = 8 + P, checksum 0.
 *        TCP  sport, dport, seq, ack = tcb[s].ack, data offset 5, tcb[s].flags, tcb[s].win,
 *             checksum 0, urgent 0. seq = tcb[s].seq + the sum of P over the MUX_PLANNED records of
 *             the same socket with a lower k, mod 2^32 (send_next += seg->size, src/tcp.c:633).
 *        The L4 checksum field is left 0 on purpose: ip_tx_frame_l4_dev and ip_tx_tso_dev fill it in
 *        the launch that frames.
 *   6. Placement. off[k] is the exclusive sum of roundup(len, align) over the planned records below
 *      k; len[k] = hl + P. A record without a datagram has len[k] = 0 and off[k] = the running
 *      offset. The framing calls answer a len of 0 with TXF_BAD_HDR and no frame, so the n-entry
 *      arrays go straight into ether_tx_frame_plan_dev / ip_tx_tso_plan_dev without a compaction or a
 *      host sync. l2[k] = {neighbour mac, route mac}, zero for no datagram. counts is a u64[4]
 *      {planned, total bytes (the sum of the padded sizes), number of MUX_NO_ROUTE, number of
 *      MUX_NO_NEIGH}. tnext[S] (may be NULL): for a TCP socket with a tcb, tcb[s].seq plus the
 *      socket's planned payload bytes mod 2^32; 0 for every other socket.
 *   7. The header image. The plan stores himg[k]: 40 bytes at stride 40 holding the finished IP and L4
 *      header; the bytes behind hl are zero, and the whole image of a record without a datagram. The
 *      caller allocates dgram only after the plan, from counts[1]; the build needs neither the tables
 *      nor the tcb.
 *   8. Build. A datagram with off[k] + len[k] > dgram_bytes is not written and gets MUX_NO_ROOM;
 *      every other planned datagram is written whole and gets MUX_BUILT. Every byte of a built
 *      datagram is stored exactly once; the pad up to align and everything outside built datagrams
 *      is not touched; no dword is read, modified and written back. For any plan arrays, nothing
 *      outside q and the plan arrays is read and nothing outside dgram and the status array is
 *      written: the build re-checks rule 1 on the record and requires that off[k] is a multiple of
 *      align, that hl (from the image's protocol byte) is 28 or 40 and that len[k] == hl + buf_size;
 *      otherwise the datagram is MUX_NO_ROOM.
 *   9. The result is a function of the inputs alone, never of scheduling.
 *
 * The input is socket-major, so the per-socket order that demux had to make with a stable partition
 * is given here: ids and sequence numbers are prefix sums over k, and no sort is needed.
 *
 * The device plan. One record or one table entry per thread; no workgroup waits for another, data
 * passes between phases only across kernel boundaries, and every probe loop is bounded by the table
 * size. Launches: (1) neighbour table, N threads, open addressing with at least 2 N entries,
 * atomicCAS claims the address and atomicMin of the index settles duplicates; (2) classify: the
 * socket of k by a bounded binary search over sfirst, rules 1-4 with the route table staged in LDS
 * and walked in index order, the counters by ballot and one atomic add per workgroup (integer adds);
 * (3) the block totals of three sums (bytes as u64, planned count, TCP payload mod 2^32), with the
 * in-block prefixes kept; (4) a one-workgroup scan of the block totals; (5) place: off, len, l2, the
 * id rank, the seq offset (the scan value at k minus the scan value at sfirst[s]) and the 40-byte
 * image with the IP checksum; (6) tnext, one thread per socket.
 * Scratch comes from one hipMallocAsync: at most MUX_SCRATCH_PER_N bytes per n plus MUX_SCRATCH_PER_S
 * per S (nothing is kept per socket) plus MUX_SCRATCH_PER_NB per N plus MUX_SCRATCH_FIXED.
 *
 * LIMITS. No gateway. Exact-match neighbours. Stateless TCP: no retransmit list, no window; tnext is
 * the only state handed back. One batch: ids and sequence numbers are carried across batches by the
 * caller, through id0 and tcb.
 *
 * Errors: -EINVAL (align, S, R, N out of range, a non-monotone sfirst in the host forms, NULL array
 * with n > 0, a misaligned q, himg or dgram in the device forms), decided before any device call,
 * text from fcs_last_error(). -ENOSPC from the host form where dgram_bytes is too small (nothing is
 * written then). Without a usable gfx950 GPU every device form and ip_tx_mux_host return -ENODEV (no
 * CPU path). Each call is thread-safe; device forms are asynchronous on `stream`. The FCS engine's
 * host-batch and fallback counters are not touched.
 */
#ifndef NSTACK_MUX_H
#define NSTACK_MUX_H

#include <stdint.h>

#include "nstack_txf.h" /* struct txf_l2 */

#ifdef __cplusplus
extern "C" {
#endif

#define MUX_BAD_REC    0x001u   /* rule 1 */
#define MUX_BAD_SIZE   0x002u   /* rule 2 */
#define MUX_NO_TCB     0x004u   /* rule 2 */
#define MUX_NO_ROUTE   0x008u   /* rule 3 */
#define MUX_NO_NEIGH   0x010u   /* rule 4 */
#define MUX_PLANNED    0x020u   /* rule 5: the plan gave it a datagram */
#define MUX_NO_ROOM    0x040u   /* rule 8 */
#define MUX_BUILT      0x080u   /* rule 8 */

#define MUX_MAX_SOCKS   65536u
#define MUX_MAX_ROUTES  256u
#define MUX_MAX_NEIGH   65536u
#define MUX_REC_HDR     24u
#define MUX_IMG         40u      /* bytes of a header image */
#define MUX_UDP_MAX     65506u   /* the largest UDP payload (src/udp.c:182) */
#define MUX_TCP_MAX     65495u   /* the largest TCP payload: 65535 - 40 */

/* the device plan's scratch bound */
#define MUX_SCRATCH_PER_N   25u
#define MUX_SCRATCH_PER_S   0u
#define MUX_SCRATCH_PER_NB  48u
#define MUX_SCRATCH_FIXED   1024u

struct mux_tcb { uint32_t seq, ack; uint16_t win; uint8_t flags, pad; };
struct mux_route { uint32_t network, netmask, gw, iface; uint8_t mac[6]; uint16_t pad; };
struct mux_neigh { uint32_t addr; uint8_t mac[6]; uint16_t valid; };

/* Host arithmetic, no GPU. Returns the planned count. mstat, off, len, l2: n entries; himg: 40 n
 * bytes; tnext: S entries or NULL; counts: 4 entries or NULL. counts[1] sizes dgram. */
int64_t ip_tx_mux_plan_host(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                            const uint64_t *bind, uint32_t S, const struct mux_tcb *tcb, const struct mux_route *rt, uint32_t R,
                            const struct mux_neigh *nb, uint32_t N, uint32_t id0, uint32_t align, uint32_t *mstat, uint64_t *off,
                            uint32_t *len, struct txf_l2 *l2, void *himg, uint32_t *tnext, uint64_t *counts);

/* Device plan: the same arrays in device memory (the tables too); counts is required. */
int ip_tx_mux_plan_dev(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                       const uint64_t *bind, uint32_t S, const struct mux_tcb *tcb, const struct mux_route *rt, uint32_t R,
                       const struct mux_neigh *nb, uint32_t N, uint32_t id0, uint32_t align, uint32_t *mstat, uint64_t *off,
                       uint32_t *len, struct txf_l2 *l2, void *himg, uint32_t *tnext, uint64_t *counts, void *stream);

/* Device build, on arrays the plan left: pstat is the plan's word, mstat gets the final one (it may be
 * pstat itself, or NULL). */
int ip_tx_mux_dev(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint32_t *pstat, const uint64_t *off,
                  const uint32_t *len, const void *himg, uint32_t align, void *dgram, uint64_t dgram_bytes, uint32_t *mstat,
                  void *stream);

/* Host batch: host memory in and out, planned on the host and built on the GPU in pipeline chunks of
 * consecutive records. Returns the planned count, or -ENOSPC where a datagram has no room in
 * dgram_bytes (nothing is written then). Any of mstat, off, len, l2, himg, tnext, counts may be NULL. */
int64_t ip_tx_mux_host(const void *q, uint64_t q_bytes, const uint64_t *rec, uint64_t n, const uint64_t *sfirst,
                       const uint64_t *bind, uint32_t S, const struct mux_tcb *tcb, const struct mux_route *rt, uint32_t R,
                       const struct mux_neigh *nb, uint32_t N, uint32_t id0, uint32_t align, void *dgram, uint64_t dgram_bytes,
                       uint32_t *mstat, uint64_t *off, uint32_t *len, struct txf_l2 *l2, void *himg, uint32_t *tnext,
                       uint64_t *counts);

/* Introspection for the tests: the kernel the last build launch of this process took ("mux", "none");
 * returns the name's length or -EINVAL. And the records of each chunk of the calling thread's last
 * ip_tx_mux_host; returns their number. */
int fcs_debug_mux_last_launch(char *out, uint64_t cap);
int64_t fcs_debug_mux_last_host_chunks(uint64_t *recs, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_MUX_H */
