/*
 * nstack_tso.h — C ABI of one-pass TCP segmentation (same library, libnstack_fcs.so).
 *
 * The build of nstack_txd.h in which a large TCP datagram leaves as MSS-sized TCP segments, each
 * with its own IP header, sequence number, flags and TCP checksum, instead of as IP fragments. The
 * reference has no such step: tcp_send_segments hands a segment of any size to ip_send
 * (src/tcp.c:614-644), ip_send fragments it (src/ip.c:326-340), and the TCB's mss (src/tcp.c:65,
 * :570, TCP_MSS at :23) never cuts a send. Segmentation is therefore NEW BEHAVIOUR throughout (what
 * a NIC's TSO does); the rules below that restate the reference carry its lines. An OPT-IN entry
 * point: nstack's sources stay untouched, and everything that is not segmented is nstack_txd.h's
 * output byte for byte, so a mixed batch is one call and needs no host partition.
 *
 * Rules for datagram i (status word bits in capitals):
 *   1. Framing rules 1-2 of nstack_txf.h hold first: TXF_BAD_HDR, TXF_BAD_LEN.
 *   2. Eligible (new behaviour) is a datagram with all of:
 *        ip_proto == 6;
 *        ntohs(ip_foff) & 0x3fff == 0 (not itself a fragment, src/nstack_ip.h:212-215; DF may be set);
 *        L = D - hlen >= 20, thl = (seg[12] >> 4) * 4 with 20 <= thl <= L (the data offset,
 *          src/tcp.h:54-55);
 *        hlen + thl <= 114. A DESIGN LIMIT: the 128-byte header image every frame is built from holds
 *          14 + hlen + thl bytes. It covers every option-free IP header (hlen 20) with any TCP options
 *          (thl <= 60), and IP options as long as the two headers together stay within 114 bytes;
 *        seg[13] & (SYN | RST | URG) == 0 (src/tcp.h:57-64 as they lie on the wire: FIN 0x01,
 *          SYN 0x02, RST 0x04, PSH 0x08, ACK 0x10, URG 0x20, ECE 0x40, CWR 0x80);
 *        cap = mtu - hlen - thl >= 1.
 *      The effective MSS is m = min(mss_i ? mss_i : cap, cap): a NULL mss array or a zero entry means
 *      "as large as the mtu allows". The payload is P = L - thl.
 *   3. Segmented (TSO_SEGMENTED; new behaviour) is an eligible datagram with P > m. It gets
 *      cnt = ceil(P / m) frames; TXF_WHOLE, TXF_FRAGMENTED, TXF_REFRAG and TXF_DF_DROP stay clear, and
 *      DF is honoured by construction: no fragment is produced. A datagram with D <= mtu but P > mss_i
 *      is segmented. EVERY OTHER datagram follows nstack_txd.h word for word (the same frames, status
 *      bits and L4 work): non-TCP, TCP that fits, ineligible TCP, an input that is itself a fragment.
 *   4. Segment s (new behaviour) carries payload bytes [s m, s m + plen_s), plen_s = min(m, P - s m),
 *      behind the datagram's own hlen IP header bytes and thl TCP header bytes; the options of both go
 *      into every segment. In its headers
 *        ip_len    = htons(hlen + thl + plen_s);
 *        ip_id     = htons((id0 + s) & 0xffff); with TSO_F_ID_FIXED id0 in every segment;
 *        ip_foff   is kept as it lies;
 *        ip_csum   follows framing rule 7 (ip_checksum over the header with the field zero, stored
 *                  as src/ip.c:79-80 stores it);
 *        tcp_seqno = htonl(seq0 + s m), modulo 2^32;
 *        FIN and PSH are cleared in every segment but the last, CWR in every segment but the first;
 *        every other TCP header byte is copied;
 *        the TCP checksum is nstack_txs.h rule 6 (tcp_checksum, src/tcp.c:167-213, stored as
 *                  tcp.c:298-299) over the thl + plen_s bytes of this segment, with that length in the
 *                  pseudo header. Whatever the field held before is ignored.
 *   5. Frame build and placement follow framing rules 8-9 (src/linux/ether.c:222-263): padding when
 *      hlen + thl + plen_s < 56; slot >= min_slot(mtu, flags), unchanged; the datagram owns slots
 *      [first[i], first[i] + cnt); TXF_NO_ROOM as before (the datagram then keeps TSO_SEGMENTED and
 *      its protocol bits only). No other byte of `out` is written. The datagram arena is never written.
 *   6. Status of a segmented datagram: TSO_SEGMENTED | TXD_L4_CSUM_SET | 6 << TXD_PROTO_SHIFT. The
 *      plan call writes the same word (for every datagram: the TXF_*, TXD_* and protocol bits of
 *      nstack_txd.h rule 4), without TXF_NO_ROOM, which only the build can know.
 *   7. Determinism: as nstack_txd.h rule 6, the result is a function of the input alone.
 * Every frame of a segmented datagram, at F + 4 bytes with TXF_F_FCS, passes ether_rx_validate_*
 * with RXV_F_TRAILER: it reads RXV_L4_CHECKED, neither RXV_FRAG nor RXV_L4_BAD_CSUM, and its only
 * possible defect bit is RXV_IP_BAD_LEN, on padded frames.
 *
 * There is no CPU path, as for nstack_txd.h: without a usable gfx950 GPU the plan, device and host
 * forms return -ENODEV, HIP errors are returned (-ENOMEM, -EIO), never answered on the host, and the
 * FCS engine's host-batch and fallback counters are not touched. Errors: 0 (host form: the frame
 * count) or -errno; -EINVAL for unknown flag bits, bad geometry and null arrays (mss may be NULL),
 * decided before any device call; -ENOSPC and the chunk bound of the host form as in nstack_txf.h;
 * text in fcs_last_error(). Thread-safe.
 */
#ifndef NSTACK_TSO_H
#define NSTACK_TSO_H

#include <stdint.h>

#include "nstack_txd.h"

#ifdef __cplusplus
extern "C" {
#endif

/* flags: those of nstack_txd.h with their values, plus */
#define TSO_F_ID_FIXED   0x200u  /* every segment keeps the datagram's ip_id */
#define TSO_F_MSS_ONE    0x400u  /* mss[0] serves the whole batch, as TXF_F_L2_ONE does for l2 */

/* status bit next to the TXF_* and TXD_* ones */
#define TSO_SEGMENTED    0x400u

/* Host arithmetic, no GPU: the frames rule 3 gives a datagram of D bytes with an hlen-byte IP header,
 * a thl-byte TCP header, the TCP flags byte tcp_flags and ntohs(ip_foff) = ip_foff at this mss (0: as
 * large as the mtu allows) and mtu; 0 when it is not segmented. */
uint32_t ip_tx_tso_count(uint32_t D, uint32_t hlen, uint32_t thl, uint32_t tcp_flags, uint32_t ip_foff,
                         uint32_t mss, uint32_t mtu);

/* ether_tx_frame_plan_dev under rules 1-3: device memory (mss too, or NULL), asynchronous on `stream`;
 * first[0..n] are the exclusive prefix sums of the frame counts, first[n] the total; status may be NULL. */
int ip_tx_tso_plan_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags, uint32_t *status,
                       uint64_t *first, void *stream);

/* ip_tx_frame_l4_dev with rules 2-6: device memory (mss too, or NULL), asynchronous on `stream`, on the
 * calling thread's current device; first[] from ip_tx_tso_plan_dev or the caller's own; flen, status
 * and fcs may each be NULL. */
int ip_tx_tso_dev(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                  const struct txf_l2 *l2, const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags,
                  const uint64_t *first, void *out, uint64_t slot, uint64_t slots, uint32_t *flen,
                  uint32_t *status, uint32_t *fcs, void *stream);

/* ip_tx_frame_l4_host with rules 2-6: host memory in and out (mss too, or NULL), synchronous, frames
 * packed from slot 0 on; returns the number of frames. */
int64_t ip_tx_tso_host(const void *dgram, uint64_t dgram_bytes, const uint64_t *off, const uint32_t *len,
                       const struct txf_l2 *l2, const uint16_t *mss, uint64_t n, uint32_t mtu, uint32_t flags,
                       void *out, uint64_t slot, uint64_t slots, uint32_t *flen, uint32_t *status);

/* Introspection for the tests: the kernel the last launch of the device and host forms in this
 * process took ("tso-fcs", "tso", "none"). Returns the name's length or -EINVAL. */
int fcs_debug_tso_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_TSO_H */
