/* SPDX-License-Identifier: BSD-3-Clause
 *
 * odpg_esp.h — ESP tunnel-mode AES-GCM of a device-resident batch.
 *
 * The batch form of the reference's IPsec data path (example/ipsec_api,
 * platform/linux-generic/odp_ipsec.c, odp_ipsec_sad.c) for the one suite
 * modern deployments use: ESP in tunnel mode over IPv4 with AES-GCM (RFC 4106;
 * 128, 192 or 256-bit keys, 16-byte ICV, 8-byte IV, 4-byte salt). An outbound
 * plan encapsulates and encrypts every frame of a batch, an inbound plan
 * authenticates, decrypts and decapsulates, and the output is again an
 * ordinary batch (odpg_batch_t / odpg_tx_batch_t) for odpg_classify,
 * odpg_l3fwd, odpg_tx_prepare or odpg_gather. The host never sees a byte.
 *
 * A plan holds up to ODPG_ESP_MAX_SAS security associations. Packet i uses SA
 * src->sa[i] (or uniform_sa) and has its L3 header at src->l3_offset[i] (or
 * uniform_l3). fr is the frame, n its length, L its L3 offset, s its SA.
 *
 * Outbound (ipsec_out_tunnel_parse_ipv4/6, ipsec_out_tunnel_ipv4 :1222-1320,
 * ipsec_out_iv :1408-1457, ipsec_out_esp :1459-1667, ipsec_out_esp_post):
 *  1. s >= max_sas or SA s not set                 -> ODPG_ESP_NO_SA
 *  2. L + 20 > n                                   -> ODPG_ESP_BAD_L3
 *     version fr[L] >> 4 is 4: ihl >= 5, ip_len = be16(fr[L + 2]) >= 4 ihl,
 *       next = 4, tos = fr[L + 1], df = bit 0x4000 of the frag field;
 *     version 6: L + 40 <= n, ip_len = 40 + be16(fr[L + 4]), next = 41, tos
 *       the traffic class, df = 0;
 *     anything else, or L + ip_len > n             -> ODPG_ESP_BAD_L3
 *     Bytes beyond L + ip_len (Ethernet padding) are dropped, as the reference
 *     truncates the tail.
 *  3. E = (ip_len + 2 + 3) & ~3 (the GCM pad mask is 3, odp_ipsec_sad.c
 *     :428-436), tot = 20 + 16 + E + 16; tot > sa.mtu -> ODPG_ESP_MTU, before
 *     a sequence number is taken (:1506-1513).
 *  4. Sequence numbers. The batch is the sequential run over it in index
 *     order: seq64 = next_seq[s] + (number of OK packets j < i with SA s), and
 *     after the call next_seq[s] has advanced by the SA's OK count. Failed
 *     packets take no number (their seq[i] is 0). seq[i] is the low 32 bits.
 *     Numbers are taken whether or not the frame fits `capacity`.
 *  5. The output frame, L + tot <= n + 57 bytes: fr[0, L) unchanged; the outer
 *     IPv4 header {0x45, tos', tot, id, frag, ttl, 50, checksum, tun_src,
 *     tun_dst} with tos' = copy_dscp ? tos : (tos & 3) | dscp << 2, frag =
 *     0x4000 if (copy_df ? df : sa.df) else 0, the checksum as
 *     _odp_packet_ipv4_chksum_insert computes it; the ESP header be32(spi),
 *     be32(seq); the 8-byte IV; E bytes of ciphertext; the 16-byte ICV.
 *  6. The IV is seq64 as 8 little-endian bytes: the reference memcpy()s a
 *     uint64_t on x86 (:1422). The GCM nonce is salt | IV, the AAD the 8 bytes
 *     of the ESP header, the plaintext the inner ip_len bytes, then pad bytes
 *     1, 2, .., p with p = E - ip_len - 2, then p, then next.
 *  Deviation: with a zero frag field the reference takes the IPv4 id from
 *  per-thread blocks, which is not deterministic. Here id =
 *  be16((uint16_t)seq64) when the frag field is 0, else 0.
 *
 * Inbound (ipsec_parse_ipv4 :456-474, ipsec_in_esp :576-694, ipsec_in_esp_post
 * :696-722, ipsec_in_strip_tunnel :1024-1050):
 *  1. NO_SA as above.
 *  2. L + 20 > n, version != 4, ihl < 5, a fragment (MF set or offset != 0) or
 *     tot_len > n - L                              -> ODPG_ESP_BAD_L3
 *  3. protocol != 50                               -> ODPG_ESP_BAD_PROTO
 *  4. tot_len < 4 ihl + 16 + 16 + 2                -> ODPG_ESP_BAD_LEN
 *  5. be32(esp.spi) != sa.spi                      -> ODPG_ESP_BAD_SPI
 *     seq[i] = be32(esp.seq) for every packet that reached this step (0
 *     otherwise), so a caller can run its replay window.
 *  6. C = tot_len - 4 ihl - 32 ciphertext bytes, any length; nonce = salt |
 *     the frame's 8 IV bytes; AAD = the ESP header.
 *  7. tag differs                                  -> ODPG_ESP_AUTH
 *  8. p = pt[C - 2], next = pt[C - 1]; p + 2 > C or pt[C - 2 - p + k] != k + 1
 *     for a k < p                                  -> ODPG_ESP_BAD_PAD
 *  9. next not 4 or 41                             -> ODPG_ESP_BAD_NEXT
 * 10. The output frame is fr[0, L) | pt[0, C - 2 - p), unmodified.
 *  Deviation: with dec_ttl = 0 the reference re-inserts the inner IPv4
 *  checksum; this library leaves the inner packet as decrypted.
 *
 * Layout and capacity are odpg_gather's, as odpg_lso.h states them, with one
 * output position per packet: position i belongs to packet i and starts at the
 * sum of the reserved bytes of the positions before it. An outbound packet
 * reserves align16(L + tot), a failed one nothing. An inbound packet that
 * passes steps 1-5 reserves align16(L + C - 2), the upper bound known before
 * decryption (no second scan): a packet failing steps 7-9 leaves a hole of
 * reserved, unwritten bytes and the descriptor {offset, 0}; an OK one has its
 * true length in the descriptor, zeros up to align16 of it and the rest of
 * its reservation unwritten. dst->desc[i] = {offset, len}; a failed packet has
 * {offset, 0}. A frame is written whole or not at all: iff its reservation
 * ends at or below `capacity` and i < max_out. Those positions are a prefix of
 * total->copied positions; the other descriptors below min(num, max_out) are
 * {0, 0}. status[i] and seq[i] do not depend on capacity (an inbound packet
 * that does not fit is still authenticated). Nothing is written at or beyond
 * frames + capacity or desc + max_out. total->bytes is the full need,
 * total->num_out the number of OK packets, total->first_bad the smallest
 * failing index (num if none). A source frame is read in whole 16-byte units
 * inside [offset, offset + align16(len)).
 *
 * Not covered: transport mode, an IPv6 outer header, AH, UDP encapsulation,
 * ESN, TFC padding; dec_ttl, anti-replay state, lifetimes and statistics;
 * inner checksum insertion (run odpg_tx_prepare first); other algorithms; the
 * Ethertype of fr[0, L), which is the caller's to fix for an IPv6 inner frame,
 * as in the reference.
 */
#ifndef ODPG_ESP_H_
#define ODPG_ESP_H_

#include "odpg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 2048 SAs and the bucket of failed packets: the key of the radix partition
 * (radix_pass.h) that ranks a batch's packets per SA. Up to 2047 SAs it is one
 * digit and one pass. */
#define ODPG_ESP_MAX_SAS 2048u
#define ODPG_ESP_OUT 0u
#define ODPG_ESP_IN  1u

/* status[i] */
#define ODPG_ESP_OK        0u
#define ODPG_ESP_NO_SA     1u
#define ODPG_ESP_BAD_L3    2u
#define ODPG_ESP_MTU       3u   /* outbound */
#define ODPG_ESP_BAD_PROTO 4u   /* inbound, and below */
#define ODPG_ESP_BAD_SPI   5u
#define ODPG_ESP_BAD_LEN   6u
#define ODPG_ESP_AUTH      7u
#define ODPG_ESP_BAD_PAD   8u
#define ODPG_ESP_BAD_NEXT  9u

/* Packets one workgroup of the crypt kernel handles (esp.hip). Informative:
 * batches are of any size; sizes around multiples of it are where the kernel
 * changes shape. */
#define ODPG_ESP_TILE 16u

typedef struct odpg_esp_sa_s {
	uint32_t spi;
	uint8_t  key[32];
	uint32_t key_len;              /* 16, 24 or 32 */
	uint8_t  salt[4];
	uint8_t  tun_src[4], tun_dst[4];
	uint8_t  ttl, dscp, df, copy_dscp, copy_df;
	uint8_t  reserved;
	uint16_t mtu;                  /* outer IPv4 tot_len limit (outbound) */
} odpg_esp_sa_t;

typedef struct odpg_esp_s odpg_esp_t;

typedef struct odpg_esp_src_s {
	const uint8_t     *frames;     /* device */
	const odpg_desc_t *desc;       /* device, or NULL: fixed stride, len = stride */
	uint32_t           stride;     /* multiple of 16 when desc == NULL */
	uint32_t           num;
	const uint16_t    *sa;         /* device, one per packet, or NULL: uniform_sa */
	const uint16_t    *l3_offset;  /* device, one per packet, or NULL: uniform_l3 */
	uint16_t           uniform_sa;
	uint16_t           uniform_l3;
	uint32_t           reserved;
} odpg_esp_src_t;

typedef struct odpg_esp_total_s {  /* device, written by every call */
	uint32_t num_out;    /* OK packets */
	uint32_t copied;     /* positions written: the longest prefix that fits */
	uint32_t first_bad;  /* smallest failing packet index, num if none */
	uint32_t reserved;   /* 0 */
	uint64_t bytes;      /* bytes the whole batch needs */
} odpg_esp_total_t;

typedef struct odpg_esp_dst_s {
	uint8_t          *frames;     /* device */
	uint64_t          capacity;   /* bytes writable at frames; <= 2^32 */
	odpg_desc_t      *desc;       /* device, max_out entries */
	uint32_t          max_out;
	uint32_t          reserved;
	uint8_t          *status;     /* device, src->num bytes */
	uint32_t         *seq;        /* device, src->num words */
	odpg_esp_total_t *total;      /* device */
} odpg_esp_dst_t;

/* The AES key expansion (FIPS-197: 4 (Nr + 1) big-endian words, Nr = 10, 12 or
 * 14; the rest of rk is zeroed) and the GHASH key H = AES_K(0^128). Host only,
 * no device needed. -EINVAL for a null pointer or a key_len other than 16, 24
 * or 32. */
int  odpg_esp_key_schedule(const uint8_t *key, uint32_t key_len, uint32_t rk[60], uint8_t h[16]);

/* Plan: dir is ODPG_ESP_OUT or ODPG_ESP_IN, max_sas 1 to ODPG_ESP_MAX_SAS (no
 * SA set yet), max_pkts at most 2^24. -EINVAL outside those. Holds a context
 * reference like counters do (odpg.h "object lifetimes"). */
int  odpg_esp_create(odpg_ctx_t *ctx, uint32_t dir, uint32_t max_sas, uint32_t max_pkts,
		     odpg_esp_t **plan);
void odpg_esp_destroy(odpg_esp_t *plan);

/* Sets SA `index` (NULL clears it): expands the key on the host, computes H
 * and its powers H^1 .. H^16 and uploads them, ordered with the calls on the
 * context stream; an outbound plan's next_seq[index] becomes 1, the
 * reference's initial value. -EINVAL for a null plan, index >= max_sas or a
 * bad key_len. */
int  odpg_esp_sa_set(odpg_esp_t *plan, uint32_t index, const odpg_esp_sa_t *sa);

/* The device address of the outbound sequence counters, max_sas 64-bit words.
 * Between batches a caller saves or preloads them with odpg_memcpy_d2h /
 * odpg_memcpy_h2d. NULL for a null or inbound plan. */
uint64_t *odpg_esp_next_seq(odpg_esp_t *plan);

/* Asynchronous on the context stream; allocates nothing; no host sync.
 * num == 0 writes *total only. -EINVAL, with nothing launched, for a null
 * plan, src, dst, dst->frames, dst->status, dst->seq or dst->total (or
 * dst->desc with max_out != 0, or src->frames with src->num != 0), a frames
 * pointer that is not 16-byte aligned, an sa or l3_offset pointer that is not
 * 2-byte aligned, src->num > max_pkts, a fixed stride that is zero or no
 * multiple of 16, and capacity > 2^32. One call at a time per plan. */
int  odpg_esp(odpg_esp_t *plan, const odpg_esp_src_t *src, const odpg_esp_dst_t *dst);

#ifdef __cplusplus
}
#endif

#endif /* ODPG_ESP_H_ */
