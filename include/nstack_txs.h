/*
 * nstack_txs.h — C ABI of one-pass TX sealing (same library, libnstack_fcs.so).
 *
 * Sealing a frame writes its IPv4 header checksum, its TCP / UDP / ICMP checksum and its FCS into
 * it, so that it is ready for the wire: what the reference does per frame in ip_hton
 * (src/ip.c:79-80), tcp_hton (src/tcp.c:298-299), src/icmp.c:41-42 and ether_send
 * (src/linux/ether.c:262-263). One launch reads every frame of a batch once, as it will lie on the
 * wire (after every hton), and stores the fields in place. The mirror image of nstack_rxv.h; an
 * OPT-IN entry point: nstack's sources stay untouched.
 *
 * len[i] is the number of covered bytes F and excludes the FCS. With TXS_F_FCS the four bytes
 * behind the frame, [F, F + 4), belong to it: they must lie inside the arena, and frames and their
 * FCS places must not overlap one another (the contract of ether_fcs_tx_batch_host).
 *
 * Rules for frame i of F bytes (status word bits in capitals):
 *   1. TXS_RUNT         F < 14; no L3 or L4 work. Otherwise P = F - 14 payload bytes start at
 *                       frame byte 14.
 *   2. TXS_IPV4         frame bytes 12, 13 (big-endian) == 0x0800; otherwise no L3 or L4 work.
 *   3. TXS_IP_BAD_HDR   the validator's rule 4 with this P: hlen = (vhl & 0x0f) * 4; set, and
 *                       nothing in L3 or L4 is written, when P < 20, or (vhl & 0x40) != 0x40
 *                       (src/ip.c:130, quirk kept), or hlen < 20, or hlen > P. Otherwise ip_proto
 *                       goes to bits 16..23 and the IP checksum is written at frame bytes 24, 25:
 *                       ip_checksum(header with bytes 24, 25 taken as zero, hlen) (arithmetic of
 *                       ip.c:39-62), stored as the reference stores it (ip.c:79-80: the uint16_t
 *                       as it is, no byte swap). TXS_IP_CSUM_SET.
 *   4. TXS_IP_BAD_LEN   ntohs(ip_len) < hlen or > P; no L4 work. ip_len < P is normal on transmit
 *                       (ether_send pads to 60 bytes) and is not flagged; the padding is never
 *                       summed, but the FCS covers it.
 *   5. TXS_FRAG         ntohs(ip_foff) & 0x3fff non-zero (src/nstack_ip.h:212-215); no L4 work.
 *                       Independent of rule 4: both bits can be set.
 *   6. L4 over L = ip_len - hlen bytes from frame byte 14 + hlen; the pseudo header from the
 *      header's own address words and L:
 *        TCP (6)   L < 20: TXS_L4_SHORT. Otherwise segment bytes 16, 17 =
 *                  tcp_checksum(ntohl(src), ntohl(dst), seg with the field zero, L)
 *                  (tcp.c:167-213, stored as tcp.c:298-299).
 *        UDP (17)  L < 8: TXS_L4_SHORT. Otherwise segment bytes 6, 7 =
 *                  udp_checksum(seg with the field zero, L, src, dst) with the raw in_addr_t words
 *                  (udp.c:136-174); a result of 0 is stored as 0xffff (RFC 768). With
 *                  TXS_F_UDP_ZERO the field is set to 0 ("no checksum") instead, nothing is
 *                  summed and TXS_L4_CSUM_SET stays clear.
 *        ICMP (1)  L < 4: TXS_L4_SHORT. Otherwise message bytes 2, 3 =
 *                  ip_checksum(msg with the field zero, L) (icmp.c:41-42).
 *        other     nothing.
 *      TXS_L4_CSUM_SET when a checksum was written.
 *   7. With TXS_F_FCS: ether_fcs over the F bytes as they now stand, stored little-endian at
 *      [F, F + 4) as ether.c:262-263 does; TXS_FCS_SET. For every F (0 included) these are the
 *      bytes ether_fcs_tx_batch_host writes for the same frame bytes.
 * Whatever a checksum field holds beforehand is ignored: sealing is idempotent. No byte other than
 * the three fields and the FCS place is written, and no byte outside the frame is interpreted.
 * A sealed frame passes ether_rx_validate_* (with RXV_F_TRAILER over F + 4 bytes) with no defect
 * bit other than RXV_IP_BAD_LEN for padded frames.
 *
 * There is no CPU path, as for nstack_rxv.h: without a usable gfx950 GPU the entry points return
 * -ENODEV, and HIP errors are returned (-ENOMEM, -EIO), never answered on the host; the FCS
 * engine's host-batch and fallback counters are not touched. Errors: 0 (host form: the count) or
 * -errno; -EINVAL for unknown flag bits and bad geometry; text in fcs_last_error(). Thread-safe.
 */
#ifndef NSTACK_TXS_H
#define NSTACK_TXS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags */
#define TXS_F_FCS       1u  /* also write the FCS of the finished frame at [len, len + 4) */
#define TXS_F_UDP_ZERO  2u  /* UDP: write 0 ("no checksum"), as the reference effectively does (src/udp.c:192) */

/* status bits */
#define TXS_FCS_SET      0x001u
#define TXS_RUNT         0x002u
#define TXS_IPV4         0x004u
#define TXS_IP_BAD_HDR   0x008u
#define TXS_IP_BAD_LEN   0x010u
#define TXS_IP_CSUM_SET  0x020u
#define TXS_FRAG         0x040u
#define TXS_L4_CSUM_SET  0x080u
#define TXS_L4_SHORT     0x200u
#define TXS_PROTO_SHIFT  16      /* bits 16..23: ip_proto, when TXS_IPV4 is set and TXS_IP_BAD_HDR is clear */

/* What was written into frame i, 0 where nothing was: the two checksums as the uint16_t the
 * reference stores (memcpy of the two bytes in the frame), the FCS as ether_fcs returns it. */
struct txs_fields { uint16_t ip_csum, l4_csum; uint32_t fcs; };

/* ---- device-resident batches: asynchronous on `stream` (a hipStream_t or NULL), on the calling
 *      thread's current device; conventions of ether_rx_validate_dev ---- */
/* Frame i = arena[off[i] .. off[i] + len[i]) (and its FCS place with TXS_F_FCS), inside
 * [arena, arena + arena_bytes); off, len, status (n u32), fields (n records) and count are device
 * memory. status and fields may each be NULL. count may be NULL; otherwise *count is zeroed on the
 * stream and then set to the number of frames with (status[i] & count_mask) != 0. */
int ether_tx_seal_dev(void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                      uint32_t flags, uint32_t count_mask, uint32_t *status, struct txs_fields *fields,
                      uint64_t *count, uint64_t n, void *stream);
/* Frame i = base[i*stride .. i*stride + len). stride >= len (with TXS_F_FCS: len + 4) when n > 1. */
int ether_tx_seal_fixed_dev(void *base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags,
                            uint32_t count_mask, uint32_t *status, struct txs_fields *fields,
                            uint64_t *count, void *stream);

/* ---- host batch (host memory in and out; chunked H2D -> kernel -> D2H on the engine's first
 *      GPU, in the library's own staging; synchronous). Only the status word and the fields record
 *      of each frame travel back; the caller's frames are patched from them on the host. ----
 * Every frame and FCS place is checked against the arena before any work: -EINVAL names the first
 * one outside it and nothing has been written. status may be NULL. Returns the number of frames
 * with (status[i] & count_mask) != 0, or -errno. A HIP error in the middle of a batch (-ENOMEM, -EIO)
 * can leave the arena partly sealed: the chunks finished before it have been patched, status[] of the
 * others is not written. Sealing is idempotent, so the whole call can simply be repeated. */
int64_t ether_tx_seal_host(void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                           uint32_t flags, uint32_t count_mask, uint32_t *status, uint64_t n);

/* Tuning: fixed-stride batches of more than `frames` frames of 1496..1524 B whose four-frame items fit
 * a 6 KiB LDS slot (3 * stride + len <= 6126, stride <= 2048; with TXS_F_FCS stride >= len + 4) take
 * the LDS-DMA kernel, every other batch the general kernel. The bytes written are identical either
 * way. Default 16384. Returns the previous value. */
uint64_t ether_tx_seal_set_dma_threshold(uint64_t frames);

/* Introspection for the tests: the kernel a fixed-stride batch would take ("lds-dma", "general",
 * "none"; host arithmetic only), and the one the last launch of this process took. Return the
 * name's length or -EINVAL. */
int fcs_debug_txs_route(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags, char *out, uint64_t cap);
int fcs_debug_txs_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_TXS_H */
