/*
 * nstack_txd.h — C ABI of TX framing with L4 checksums (same library, libnstack_fcs.so).
 *
 * The build of nstack_txf.h plus the TCP / UDP / ICMP checksum of every datagram, summed in the same
 * launch that frames it and stored in the frame that carries the field: what the reference does on
 * the host in nstack_udp_send (src/udp.c:176-200), tcp_hton (src/tcp.c:287-300) and icmp.c:41-42
 * before ip_send -> ip_send_fragments -> ether_send (src/ip.c:225-269, 318-340;
 * src/linux/ether.c:222-263). It removes the extra pass nstack_txf.h rule 10 asks the caller for:
 * a fragmented datagram's checksum spans its fragments, so no frame-by-frame sealer (nstack_txs.h
 * rule 5) can fill it. An OPT-IN entry point: nstack's sources stay untouched. The plan stays
 * ether_tx_frame_plan_dev / ether_tx_frame_count: frame counts and slots do not change.
 *
 * Rules for datagram i (status word bits in capitals):
 *   1. Framing. Rules 1-9 of nstack_txf.h hold word for word. With the L4 field of the datagram
 *      replaced as below, the output is byte for byte what ether_tx_frame_dev writes for that
 *      datagram: frames, flen, fcs, the TXF_* status bits, TXF_NO_ROOM, and untouched bytes
 *      everywhere else in `out`. The datagram arena is never written.
 *   2. L4 work only for a datagram that becomes frames and whose own ntohs(ip_foff) & 0x3fff is
 *      zero (src/nstack_ip.h:212-215). An input that is itself a fragment and is framed TXF_WHOLE
 *      gets none, as nstack_txs.h rule 5 says: its bytes are ether_tx_frame_dev's.
 *   3. The checksum: nstack_txs.h rule 6 word for word over the L = D - hlen segment bytes (framing
 *      rule 2 has made ip_len == D); the pseudo header from the header's own address words and L:
 *        TCP (6)   L < 20: TXD_L4_SHORT. Otherwise segment bytes 16, 17 =
 *                  tcp_checksum(ntohl(src), ntohl(dst), seg with the field zero, L)
 *                  (tcp.c:167-213, stored as tcp.c:298-299).
 *        UDP (17)  L < 8: TXD_L4_SHORT. Otherwise segment bytes 6, 7 =
 *                  udp_checksum(seg with the field zero, L, src, dst) with the raw in_addr_t words
 *                  (udp.c:136-174); a result of 0 is stored as 0xffff (RFC 768). With
 *                  TXD_F_UDP_ZERO the field is set to 0 ("no checksum", src/udp.c:192) instead,
 *                  nothing is summed and TXD_L4_CSUM_SET stays clear.
 *        ICMP (1)  L < 4: TXD_L4_SHORT. Otherwise message bytes 2, 3 =
 *                  ip_checksum(msg with the field zero, L) (icmp.c:41-42).
 *        other     nothing.
 *      Whatever the field holds beforehand is ignored. The IP header bytes and the padding of
 *      framing rule 8 are not part of the sum.
 *   4. Status word: the TXF_* bits of nstack_txf.h, TXD_L4_CSUM_SET when a checksum was written,
 *      TXD_L4_SHORT, and ip_proto in bits 16..23 when the datagram passed framing rules 1 and 2
 *      (TXF_BAD_HDR and TXF_BAD_LEN clear), whether or not it becomes frames.
 *   5. Where the field lies: in fragment fo / max of a fragmented datagram, fo = 16, 6 or 2 the
 *      field's offset in the segment and max the payload unit of framing rule 6. That is fragment 0
 *      except for small units: at mtu 76, hlen 60 gives max = 8 and hlen 52 gives max = 16, so the
 *      TCP field lies in fragment 2 or 1. max is a multiple of 8 and fo is even, so the field never
 *      straddles fragments. With TXF_F_FCS that frame's FCS and its fcs[] entry are those of the
 *      stored bytes.
 *   6. Determinism: the result is a function of the input alone, not of scheduling, slot order or
 *      alignment.
 * After reassembly (nstack_rxr.h) every datagram rule 3 gave a checksum passes the check of
 * nstack_rxd.h: RXD_L4_CHECKED and not RXD_L4_BAD_CSUM.
 *
 * There is no CPU path, as for nstack_txf.h: without a usable gfx950 GPU the device and host forms
 * return -ENODEV, HIP errors are returned (-ENOMEM, -EIO), never answered on the host, and the FCS
 * engine's host-batch and fallback counters are not touched. Errors: 0 (host form: the frame count)
 * or -errno; -EINVAL for unknown flag bits, bad geometry and null arrays (decided before any device
 * call); -ENOSPC and the chunk bound of the host form as in nstack_txf.h; text in fcs_last_error().
 * Thread-safe.
 */
#ifndef NSTACK_TXD_H
#define NSTACK_TXD_H

#include <stdint.h>

#include "nstack_txf.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags: TXF_F_FCS, TXF_F_HONOR_DF and TXF_F_L2_ONE with their values, plus */
#define TXD_F_UDP_ZERO   0x100u  /* UDP: write 0 ("no checksum"); what TXS_F_UDP_ZERO means */

/* status bits next to the TXF_* ones (the values of their TXS_* namesakes) */
#define TXD_L4_CSUM_SET  0x080u
#define TXD_L4_SHORT     0x200u
#define TXD_PROTO_SHIFT  16      /* bits 16..23: ip_proto, when TXF_BAD_HDR and TXF_BAD_LEN are clear */

/* ether_tx_frame_dev with rules 2-5: device memory, asynchronous on `stream`, on the calling
 * thread's current device; first[] from ether_tx_frame_plan_dev or the caller's own; flen, status
 * and fcs may each be NULL. */
int ip_tx_frame_l4_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, const uint64_t *first,
                       void *out, uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status, uint32_t *fcs,
                       void *stream);

/* ether_tx_frame_host with rules 2-5: host memory in and out, synchronous, frames packed from slot
 * 0 on; returns the number of frames. */
int64_t ip_tx_frame_l4_host(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                            const struct txf_l2 *l2, uint64_t n, uint32_t mtu, uint32_t flags, void *out,
                            uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status);

/* Introspection for the tests: the kernel the last launch of these two calls in this process took
 * ("general-l4-fcs", "general-l4", "none"). Returns the name's length or -EINVAL. */
int fcs_debug_txd_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_TXD_H */
