/*
 * nstack_rxv.h — C ABI of the one-pass RX validator (same library, libnstack_fcs.so).
 *
 * One launch reads every received frame once, as it lies on the wire (before any ntoh), and
 * returns one verdict word per frame: the FCS residue test of ether_fcs_verify_*, the IPv4 header
 * checks of ip_input and the L4 checksums of tcp_input / udp_input / icmp_input. It restates the
 * reference's own predicates, including the two receive-side checksum tests the reference has
 * under "#if 0" (src/ip.c:147-155, src/tcp.c:508-515). An OPT-IN entry point:
 * nstack's sources stay untouched.
 *
 * Verdict of frame i of F bytes; T = 4 with RXV_F_TRAILER, else 0:
 *   1. RXV_FCS_BAD      with RXV_F_TRAILER: set exactly when ether_fcs_verify_* gives ok[i] == 0
 *                       (ether_fcs over all F bytes != 0x2144DF1C; frames shorter than 4 bytes
 *                       never check). Without the flag no CRC is computed and the bit is clear.
 *                       Every other bit is independent of this one.
 *   2. RXV_RUNT         F < 14 + T; nothing further. Otherwise P = F - 14 - T payload bytes start
 *                       at frame byte 14.
 *   3. RXV_IPV4         frame bytes 12, 13 (big-endian) == 0x0800 (ETHER_PROTO_IPV4); otherwise
 *                       nothing further (0x8100 and 0x86DD are "not IPv4").
 *   4. RXV_IP_BAD_HDR   hlen = (vhl & 0x0f) * 4; set, and nothing further, when P < 20, or
 *                       (vhl & 0x40) != 0x40 (src/ip.c:130, quirk kept), or hlen < 20 (ip.c:136),
 *                       or hlen > P (the header must lie inside the frame; this library's own
 *                       bound). Otherwise ip_proto goes to bits 16..23.
 *   5. RXV_IP_BAD_LEN   ntohs(ip_len) != P (ip.c:141). The reference therefore drops frames
 *                       padded to the Ethernet minimum; bad_mask lets the caller decide.
 *   6. RXV_IP_BAD_CSUM  ip_checksum(header as on the wire, hlen) != 0: the check ip.c:151
 *                       intends, with the arithmetic of ip.c:39-62.
 *   7. RXV_FRAG         ntohs(ip_foff) & 0x2000 or & 0x1fff non-zero (src/nstack_ip.h:212-215).
 *                       No L4 check follows.
 *   8. L4: L = ip_len - hlen bytes from frame byte 14 + hlen, evaluated only when
 *      hlen <= ip_len <= P (padding and trailer are never summed):
 *        TCP (6)   L < 20: RXV_L4_SHORT (src/tcp.c:496). Otherwise RXV_L4_CHECKED, and
 *                  RXV_L4_BAD_CSUM when tcp_checksum(ntohl(src), ntohl(dst), seg, L) != 0
 *                  (tcp.c:510, arithmetic of tcp.c:167-213).
 *        UDP (17)  L < 8: RXV_L4_SHORT (src/udp.c:83). Otherwise, when the checksum field (segment
 *                  bytes 6, 7) is zero the sender sent none: no check. Otherwise RXV_L4_CHECKED,
 *                  and RXV_L4_BAD_CSUM when udp_checksum(seg, L, src, dst) != 0 with the raw
 *                  in_addr_t words as they lie in the header (udp.c:136-174).
 *        ICMP (1)  L < 4: RXV_L4_SHORT. Otherwise RXV_L4_CHECKED, and RXV_L4_BAD_CSUM when
 *                  ip_checksum(msg, L) != 0 (src/icmp.c:42).
 *        other     nothing.
 * No byte outside the frame is interpreted, whatever the header fields say.
 *
 * There is no CPU path, as for the Internet checksums (nstack_inet.h): without a usable gfx950
 * GPU the entry points return -ENODEV, and HIP errors are returned (-ENOMEM, -EIO), never
 * answered on the host. Errors: 0 (host form: the bad count) or -errno; -EINVAL for unknown flag
 * bits, a NULL verdict with n > 0 and other bad arguments; text in fcs_last_error(). Thread-safe.
 */
#ifndef NSTACK_RXV_H
#define NSTACK_RXV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* flags */
#define RXV_F_TRAILER   1u   /* frames include their 4-byte FCS (as ether_fcs_verify_*): check it */

/* verdict bits */
#define RXV_FCS_BAD      0x001u
#define RXV_RUNT         0x002u
#define RXV_IPV4         0x004u
#define RXV_IP_BAD_HDR   0x008u
#define RXV_IP_BAD_LEN   0x010u
#define RXV_IP_BAD_CSUM  0x020u
#define RXV_FRAG         0x040u
#define RXV_L4_CHECKED   0x080u
#define RXV_L4_BAD_CSUM  0x100u
#define RXV_L4_SHORT     0x200u
#define RXV_PROTO_SHIFT  16      /* bits 16..23: ip_proto, when RXV_IPV4 is set and RXV_IP_BAD_HDR is clear */

/* ---- device-resident batches: asynchronous on `stream` (a hipStream_t or NULL), on the calling
 *      thread's current device; conventions of ether_fcs_verify_dev ---- */
/* Frame i = arena[off[i] .. off[i] + len[i]), inside [arena, arena + arena_bytes); off, len,
 * verdict (n u32) and bad are device memory. bad may be NULL; otherwise *bad is zeroed on the
 * stream and then set to the number of frames with (verdict[i] & bad_mask) != 0. */
int ether_rx_validate_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                          uint32_t flags, uint32_t bad_mask, uint32_t *verdict, uint64_t *bad, uint64_t n,
                          void *stream);
/* Frame i = base[i*stride .. i*stride + len). stride >= len when n > 1. */
int ether_rx_validate_fixed_dev(const void *base, uint64_t stride, uint32_t len, uint64_t n, uint32_t flags,
                                uint32_t bad_mask, uint32_t *verdict, uint64_t *bad, void *stream);

/* ---- host batch (host memory in and out; chunked H2D -> kernel -> D2H on the engine's first
 *      GPU, in the library's own staging; synchronous) ----
 * Every frame is checked against the arena before any work: -EINVAL names the first frame outside
 * it and nothing has been written. Returns the number of frames with (verdict[i] & bad_mask) != 0,
 * or -errno. */
int64_t ether_rx_validate_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                               uint32_t flags, uint32_t bad_mask, uint32_t *verdict, uint64_t n);

/* Tuning: fixed-stride batches of more than `frames` frames of 1496..1524 B whose four-frame items fit
 * a 6 KiB LDS slot (3 * stride + len <= 6126, stride <= 2048) take the LDS-DMA kernel, every other
 * batch the general kernel. Verdicts are identical either way. Default 16384. Returns the previous
 * value. */
uint64_t ether_rx_validate_set_dma_threshold(uint64_t frames);

/* Introspection for the tests: the kernel a fixed-stride batch would take ("lds-dma", "general",
 * "none"; host arithmetic only), and the one the last launch of this process took. Return the
 * name's length or -EINVAL. */
int fcs_debug_rxv_route(uint64_t base, uint64_t stride, uint32_t len, uint64_t n, char *out, uint64_t cap);
int fcs_debug_rxv_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_RXV_H */
