/*
 * nstack_dmx.h — C ABI of one-pass RX demultiplexing (same library, libnstack_fcs.so).
 *
 * nstack_rxr.h, nstack_rxd.h and nstack_gro.h turn received frames into IPv4 datagrams with an L4
 * verdict each, as the reference's ether_receive -> ip_input -> ip_fragment_input does. The reference
 * then does one more thing with a datagram: udp_input (src/udp.c:75-133) and tcp_input / tcp_fsm
 * (src/tcp.c:433-445) look up the bound socket by (ip_dst, destination port) with find_udp_socket /
 * find_tcp_socket (an exact memcmp of a struct nstack_sockaddr) and hand the payload to
 * nstack_sock_dgram_input (src/nstack.c:125-146), which appends one
 * struct nstack_dgram { srcaddr, dstaddr, buf_size, buf[] } to that socket's ingress queue. These
 * calls are that last hop on the device: datagrams in, per-socket queues of nstack_dgram records out,
 * every payload byte read once and written once, the records of one socket contiguous and in arrival
 * order. NEW and OPT-IN: nothing that exists changes a byte, a status word, a launch name or a launch.
 *
 * Inputs are the arrays ip_rx_reasm_l4_dev or ip_rx_gro_dev left: out, out_bytes, doff, dlen, dverdict
 * (may be NULL), counts (device u64[2] {m, doff[m]}) and n, the arrays' capacity; m = min(counts[0], n).
 * The host forms take m itself as n.
 *
 * The bind table bind[S], 0 <= S <= 65536, holds u64 keys proto << 48 | port << 32 | addr: proto 6 or
 * 17, the host-order port, and the host-order IPv4 address as nstack_sockaddr.inet4_addr holds it after
 * ip_ntoh (src/ip.c:93-94). A key that occurs more than once belongs to its lowest index. A key with
 * another proto, or with bits 56..63 set, is -EINVAL in the host forms and matches nothing in the
 * device forms. align is a power of two in 8..128: records start on multiples of it inside q, and the
 * device forms want q itself aligned to it. drop_mask is applied to dverdict[k].
 *
 * Rules for datagram k < m (dg = out + doff[k], D = dlen[k]; status bits of dstat[k] in capitals).
 * Entries [m, n) of every per-datagram array are zero (dstat) or "none" (dsock, rec).
 *   1. DMX_DROPPED     doff[k] + D > out_bytes; or dverdict != NULL and
 *                      dverdict[k] & (drop_mask | RXD_NO_ROOM); or D < 20; or hlen = (dg[0] & 15) * 4
 *                      outside 20..D. Nothing else is looked at.
 *   2. DMX_NO_PROTO    proto = dg[9] is neither 6 nor 17: ICMP and the rest are no socket traffic and
 *                      stay with the caller. seg = dg + hlen, L = D - hlen.
 *   3. UDP (17): DMX_SHORT when L < 8 (-EBADMSG, src/udp.c:83-87). Otherwise the payload is seg + 8 and
 *      P = L - 8; udp_len is ignored, as the reference ignores it (src/udp.c:101-103). P = 0 is queued,
 *      as the reference queues it.
 *   4. TCP (6): DMX_SHORT when L < 20 or thl = (seg[12] >> 4) * 4 lies outside 20..L. Otherwise the
 *      payload is seg + thl and P = L - thl. DMX_CTRL when P = 0 or SYN or RST is set: the segment is
 *      looked up (rule 5) and dsock[k] is set, but no record is made; the connection state machine
 *      stays with the caller.
 *      DEVIATION: the reference queues TCP payload only in TCP_ESTABLISHED with PSH | ACK and matching
 *      sequence numbers (src/tcp.c:421-424). This call is stateless, like every call here: it queues
 *      every TCP payload without a window check and leaves seq checks to the caller, who has
 *      rec[k] <-> k.
 *   5. Lookup. The key is (proto, ntohl(dg[16..19]), ntohs(seg[2..3])). dsock[k] is the lowest index
 *      of that key in bind. DMX_NO_SOCK when there is none ("port unreachable", src/udp.c:128-131; the
 *      RST path, src/tcp.c:369-374), and dsock[k] = 0xffffffff. Exact match only: there is no wildcard
 *      address, because the reference has none (a limit).
 *   6. Record. DMX_QUEUED: a datagram that passed rules 1-5 without a bit gets
 *      roundup(24 + P, align) bytes at q + rec[k]: little-endian u32 source address (host-order
 *      value), i32 source port, u32 destination address, i32 destination port, u64 buf_size = P, the
 *      P payload bytes, zero bytes to the record's end. That is struct nstack_dgram on LP64.
 *   7. Placement. Socket s owns [sbase[s], sbase[s + 1]) of q; sbase[0] = 0 and sbase is monotone;
 *      sockets without records own empty ranges. Inside its range the records of socket s lie back to
 *      back in ASCENDING k. scnt[s] is its record count. rec[k] is the record's offset, or ~0 if k
 *      made no record. qcounts is a device u64[4] {records, sbase[S], number of DMX_NO_SOCK, number of
 *      DMX_DROPPED}.
 *   8. Build. A record with rec[k] + size > q_bytes is not written, and the final word gets
 *      DMX_NO_ROOM; every other record is written whole, and the final word gets DMX_DELIVERED. Every
 *      byte of q inside a delivered record is stored exactly once, no byte outside delivered records
 *      is touched, and no dword is read, modified and written back. For any plan arrays, nothing
 *      outside `out` is read and nothing outside q and the status array is written (a rec[k] that is
 *      no multiple of align, or a datagram that fails rules 1-4 on re-check, is DMX_NO_ROOM).
 *   9. The result is a function of the inputs alone, never of scheduling.
 *
 * The device plan. Arrival order per socket without scheduling dependence is a stable partition by
 * socket index; a counter per socket taken with atomics would order records by scheduling. No
 * workgroup waits for another, data passes between phases only across kernel boundaries, and every
 * probe loop is bounded by the table size. Launches: (1) table build, S threads, open addressing with
 * at least 2 S entries, atomicCAS claims the key and atomicMin of the index settles duplicates;
 * (2) classify, one datagram per thread, rules 1-5, the record size and the counters (integer adds);
 * (3) an LSD radix pass with 8-bit digits over dsock, one when S <= 256 and two otherwise, each a
 * digit histogram per 1024-element tile, one scan launch over (digit, tile) and a scatter with an
 * in-tile stable rank from eight wave ballots per digit plus wave counts in LDS (datagrams without a
 * record are left out, which puts them behind every socket); (4) the block totals of the record sizes
 * in sorted order, their scan, and the launch that stores rec; (5) one bounded binary search per
 * socket over the sorted keys for sbase and scnt.
 * Scratch comes from one hipMallocAsync: at most DMX_SCRATCH_PER_N bytes per n plus
 * DMX_SCRATCH_PER_S per S plus DMX_SCRATCH_FIXED.
 *
 * Errors: -EINVAL (bad align, S, key, NULL array with n > 0, q not aligned), decided before any device
 * call, text from fcs_last_error(). Without a usable gfx950 GPU every device and host form returns
 * -ENODEV (no CPU path). Each call is thread-safe; device forms are asynchronous on `stream`. The FCS
 * engine's host-batch and fallback counters are not touched.
 */
#ifndef NSTACK_DMX_H
#define NSTACK_DMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMX_DROPPED    0x001u   /* rule 1 */
#define DMX_NO_PROTO   0x002u   /* rule 2 */
#define DMX_SHORT      0x004u   /* rules 3, 4 */
#define DMX_CTRL       0x008u   /* rule 4 */
#define DMX_NO_SOCK    0x010u   /* rule 5 */
#define DMX_QUEUED     0x020u   /* rule 6: the plan gave it a record */
#define DMX_NO_ROOM    0x040u   /* rule 8 */
#define DMX_DELIVERED  0x080u   /* rule 8 */

#define DMX_NONE32     0xffffffffu
#define DMX_NONE64     0xffffffffffffffffull
#define DMX_MAX_SOCKS  65536u
#define DMX_REC_HDR    24u

/* the device plan's scratch bound */
#define DMX_SCRATCH_PER_N   26u
#define DMX_SCRATCH_PER_S   48u
#define DMX_SCRATCH_FIXED   4096u

/* Host arithmetic, no GPU: n datagrams. Returns the record count. dstat, dsock, rec: n entries; sbase:
 * S + 1; scnt: S. sbase[S] sizes q. */
int64_t ip_rx_demux_plan_host(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                              const uint32_t *dverdict, uint64_t n, const uint64_t *bind, uint32_t S, uint32_t drop_mask,
                              uint32_t align, uint32_t *dstat, uint32_t *dsock, uint64_t *rec, uint64_t *sbase, uint32_t *scnt);

/* Device plan: the same arrays in device memory (bind too), plus qcounts. */
int ip_rx_demux_plan_dev(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                         const uint32_t *dverdict, const uint64_t *counts, uint64_t n, const uint64_t *bind, uint32_t S,
                         uint32_t drop_mask, uint32_t align, uint32_t *dstat, uint32_t *dsock, uint64_t *rec, uint64_t *sbase,
                         uint32_t *scnt, uint64_t *qcounts, void *stream);

/* Device build, on arrays the plan left: pstat is the plan's word, dstat gets the final one (it may be
 * pstat itself, or NULL). */
int ip_rx_demux_dev(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen, const uint64_t *counts,
                    uint64_t n, const uint32_t *pstat, const uint64_t *rec, uint32_t align, void *q, uint64_t q_bytes,
                    uint32_t *dstat, void *stream);

/* Host batch: host memory in and out, planned on the host and built on the GPU in pipeline chunks of
 * consecutive datagrams. Returns the record count, or -ENOSPC where a record has no room in q_bytes
 * (nothing is written then). Any of dstat, dsock, rec, sbase, scnt may be NULL. */
int64_t ip_rx_demux_host(const void *out, uint64_t out_bytes, const uint64_t *doff, const uint32_t *dlen,
                         const uint32_t *dverdict, uint64_t n, const uint64_t *bind, uint32_t S, uint32_t drop_mask,
                         uint32_t align, void *q, uint64_t q_bytes, uint32_t *dstat, uint32_t *dsock, uint64_t *rec,
                         uint64_t *sbase, uint32_t *scnt);

/* Introspection for the tests: the kernel the last build launch of this process took ("demux",
 * "none"); returns the name's length or -EINVAL. And the datagrams of each chunk of the calling
 * thread's last ip_rx_demux_host; returns their number. */
int fcs_debug_dmx_last_launch(char *out, uint64_t cap);
int64_t fcs_debug_dmx_last_host_chunks(uint64_t *dgs, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_DMX_H */
