/*
 * nstack_rxd.h — C ABI of RX reassembly with the L4 checksum verdict of every delivered datagram
 * (same library, libnstack_fcs.so).
 *
 * nstack_rxv.h stops at a fragment (its rule 7: "No L4 check follows"), and nstack_rxr.h "computes no
 * CRC and checks no checksum": a datagram that arrived in fragments would reach the caller with its
 * TCP/UDP/ICMP checksum unseen, although tcp_input, udp_input and icmp_input look at exactly that
 * datagram (src/tcp.c:508-515, src/udp.c, src/icmp.c:42). These calls are the build of nstack_rxr.h
 * with one verdict word per delivered datagram from the same pass over the bytes: the one's-complement
 * sum is additive, fragment offsets are multiples of 8 and header lengths multiples of 4, so every
 * fragment's payload lands on the datagram's 16-bit word grid, and the build holds every delivered
 * byte in a register between its load and its store. An OPT-IN entry point: nstack's sources stay
 * untouched, and ether_rx_reasm_* keeps its bytes, status words, launch name and symbols.
 *
 * The plan is nstack_rxr.h's (ether_rx_reasm_plan_dev / ether_rx_reasm_plan_host); the bytes of `out`
 * and the final fstat are identical to ether_rx_reasm_dev's for the same plan (its rules 7 and 8).
 *
 * Rules for delivered datagram k (verdict word bits in capitals):
 *   1. RXD_NO_ROOM     doff[k] + dlen[k] > out_bytes: the datagram was not written (RXR_NO_ROOM on its
 *                      frames, nstack_rxr.h rule 8). No other bit is set, nothing of `out` is read.
 *   2. Otherwise D = dlen[k] bytes lie at out + doff[k], exactly as ether_rx_reasm_dev writes them.
 *      hlen = (byte 0 & 0x0f) * 4, proto = byte 9 (bits 16..23 of the word, RXD_PROTO_SHIFT), the
 *      address words are bytes 12..15 and 16..19 as they lie, L = D - hlen.
 *   3. nstack_rxv.h rule 8, word for word, with D in the place of ip_len:
 *      RXD_L4_SHORT    TCP (6): L < 20. UDP (17): L < 8. ICMP (1): L < 4. Nothing is checked.
 *      RXD_L4_CHECKED  TCP: tcp_checksum(ntohl(src), ntohl(dst), seg, L) was evaluated (src/tcp.c:508-515).
 *                      UDP: the checksum field (segment bytes 6, 7) is not zero and
 *                      udp_checksum(seg, L, src, dst) was evaluated with the raw address words
 *                      (src/udp.c); a zero field means "no checksum": not checked, not bad.
 *                      ICMP: ip_checksum(msg, L) was evaluated (src/icmp.c:42).
 *      RXD_L4_BAD_CSUM the evaluated function returned non-zero.
 *      Any other protocol gets the proto bits only.
 *      The IP header is not part of any of these sums: its bytes (TTL, the header checksum, options)
 *      do not change the verdict; the address words enter through the pseudo header.
 *   4. The verdict is a function of the delivered bytes alone: not of the fragmentation, the frames'
 *      order or alignment, the address or alignment of `out`, or scheduling.
 *
 * The device form takes the arrays of ether_rx_reasm_dev as a plan call left them, and counts, the
 * device u64[2] {m, doff[m]} that ether_rx_reasm_plan_dev wrote: it is required here, because the
 * verdict launch must know m and no host value of it exists. dverdict is device memory of n u32: it
 * is zeroed on the stream (the build adds up in it), and entries [0, m) then get the verdict words;
 * entries [m, n) stay zero. bad may be NULL; otherwise it (a device u64) is zeroed on the stream and
 * then set to the number of k < m with (dverdict[k] & bad_mask) != 0, the convention of
 * ether_rx_validate_dev. Two launches behind the memsets: the build with sums (every frame adds the
 * folded sum of the bytes it stores to its datagram's word, one integer atomic add per frame: integer
 * adds commute, so nothing depends on their order) and the verdict launch (one thread per datagram:
 * it reads the delivered header back, takes its sum out, and adds the pseudo header). Data passes
 * from one to the other only across the kernel boundary.
 * A plan that a plan call did not write keeps the build's guarantees: nothing outside the frames is
 * read (of `out`, only delivered headers inside [out, out + out_bytes)), and nothing outside `out`,
 * fstat, dverdict and bad is written. Its verdict words are then unspecified.
 *
 * The host form is ether_rx_reasm_host with the verdicts: same plan, same chunks (the introspection
 * call fcs_debug_rxr_last_host_chunks of nstack_rxr.h reports them), build plus verdict launch per
 * chunk, the chunk's verdict words come back with its datagrams, bad is counted on the host. It
 * returns m; dverdict has n entries of host memory ([0, m) are written), bad is a host word or NULL.
 * It returns -ENOSPC where ether_rx_reasm_host does, so RXD_NO_ROOM never appears in it.
 *
 * No CPU path, as for nstack_rxr.h: without a usable gfx950 GPU both forms return -ENODEV, and HIP
 * errors are returned (-ENOMEM, -EIO), never answered on the host. Errors: 0 (host form: m) or -errno;
 * -EINVAL for unknown flag bits, an align that is no power of two in 1..128 (host form), NULL arrays
 * with n > 0, NULL counts (device form), NULL dverdict with n > 0 and n >= 2^30, all decided before
 * any device call; text in fcs_last_error(). Thread-safe.
 */
#ifndef NSTACK_RXD_H
#define NSTACK_RXD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* datagram verdict bits: the L4 bits have the values of nstack_rxv.h's and mean the same */
#define RXD_NO_ROOM      0x002u   /* the datagram was not written (RXR_NO_ROOM); no other bit is set */
#define RXD_L4_CHECKED   0x080u
#define RXD_L4_BAD_CSUM  0x100u
#define RXD_L4_SHORT     0x200u
#define RXD_PROTO_SHIFT  16       /* bits 16..23: ip_proto of the delivered header */

/* Device-resident batches: asynchronous on `stream` (a hipStream_t or NULL), on the calling thread's
 * current device; every array is device memory. flags: RXR_F_TRAILER of nstack_rxr.h. */
int ip_rx_reasm_l4_dev(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len, uint64_t n,
                       uint32_t flags, const uint32_t *pstat, const uint64_t *dst, const uint32_t *dgi,
                       const uint64_t *doff, const uint32_t *dlen, const uint64_t *counts,
                       void *out, uint64_t out_bytes, uint32_t *fstat,
                       uint32_t bad_mask, uint32_t *dverdict, uint64_t *bad, void *stream);

/* Host batch (host memory in and out; synchronous). */
int64_t ip_rx_reasm_l4_host(const void *arena, uint64_t arena_bytes, const uint64_t *off, const uint32_t *len,
                            uint64_t n, uint32_t flags, const uint32_t *verdict, uint32_t drop_mask, uint32_t align,
                            void *out, uint64_t out_bytes, uint32_t *fstat, uint64_t *doff, uint32_t *dlen,
                            uint32_t *dlead, uint32_t bad_mask, uint32_t *dverdict, uint64_t *bad);

/* Introspection for the tests: the kernel the last build launch with sums of this process took
 * ("general-l4", "none"). Returns the name's length or -EINVAL. */
int fcs_debug_rxd_last_launch(char *out, uint64_t cap);

#ifdef __cplusplus
}
#endif

#endif /* NSTACK_RXD_H */
