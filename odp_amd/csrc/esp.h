/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch interface of the ESP kernels (runtime.hip -> esp.hip;
 * include/odpg_esp.h is the public side) and the AES / GF(2^128) primitives
 * the host's SA setup and the kernels share. Not part of the ABI.
 *
 * Conventions. An AES state and a GHASH element are four big-endian words:
 * word 0 holds bytes 0-3, its most significant bit is GCM's bit 0 (the
 * coefficient of x^0 in GCM's reflected convention).
 */
#ifndef ODPG_ESP_INTERNAL_H_
#define ODPG_ESP_INTERNAL_H_

#include <stdint.h>
#include "../../include/odpg_esp.h"
#include "deliver.h"   /* the radix partition's tile and digit widths */

#define ESP_TILE    ODPG_ESP_TILE   /* packets per crypt workgroup */
#define ESP_GROUP   16u             /* lanes per packet: blocks of a chunk */
#define ESP_PREP_WG 256u            /* packets per prepare / place workgroup */
#define ESP_NPOW    ESP_GROUP       /* H^1 .. H^16 */

#define ESP_SA_VALID     1u
#define ESP_SA_DF        2u
#define ESP_SA_COPY_DSCP 4u
#define ESP_SA_COPY_DF   8u

/* an SA on the device: 528 bytes, the first ESP_SA_LDS_WORDS words staged in LDS */
typedef struct odpg_esp_sa_dev {
	uint32_t rk[60];               /* round keys, big-endian words */
	uint32_t hpow[ESP_NPOW][4];    /* hpow[k] = H^(k + 1) */
	uint32_t nr;                   /* rounds: 10, 12 or 14 */
	uint32_t salt;                 /* big-endian word */
	uint32_t spi;
	uint32_t flags;                /* ESP_SA_* */
	uint32_t tun_src, tun_dst;     /* big-endian words */
	uint32_t ttl_dscp;             /* ttl | dscp << 8 */
	uint32_t mtu;
} odpg_esp_sa_dev;

#define ESP_SA_LDS_WORDS (60u + 4u * ESP_NPOW)

/* what the prepare kernel leaves per packet (16 bytes) */
typedef struct odpg_esp_rec {
	uint32_t off;      /* source descriptor offset (0 with a fixed stride) */
	uint32_t l_len;    /* L | (outbound: ip_len, inbound: C) << 16 */
	uint32_t sa_st;    /* SA | status << 16 | (outbound: tos, inbound: ihl) << 24 */
	uint32_t out_fl;   /* reserved output bytes | ESP_REC_* << 24 */
} odpg_esp_rec;

#define ESP_REC_V6 1u   /* outbound: the inner packet is IPv6 */
#define ESP_REC_DF 2u   /* outbound: the inner IPv4 header has DF */

#define ESP_NOFIT 0xFFFFFFFFu   /* ounit[i] of a position that is not written */

typedef struct odpg_esp_args {
	odpg_esp_src_t src;
	odpg_esp_dst_t dst;
	uint32_t dir, max_sas;
	const odpg_esp_sa_dev *sas;   /* [max_sas] */
	const uint32_t *te0;          /* [256] the AES T-table */
	uint64_t *next_seq;           /* [max_sas], outbound */
	/* plan workspace */
	odpg_esp_rec *rec;            /* [max_pkts] */
	uint32_t *ounit;              /* [max_pkts] first output unit, ESP_NOFIT */
	uint64_t *seq64;              /* [max_pkts], outbound */
	uint64_t *tunits;             /* [tiles] 16-byte units of a tile, then of the tiles before */
	uint32_t *tok, *tbad;         /* [tiles] OK packets, smallest failing index */
	uint32_t *skey;               /* [max_pkts] partition keys, outbound: SA or max_sas */
	uint32_t *order, *offsets;    /* [max_pkts], [max_sas + 2] */
	uint32_t key_bits;
	uint32_t *hist, *dtotal, *bcount, *pairs;   /* radix_pass.h */
} odpg_esp_args;

#ifdef __HIPCC__
#define ESP_HD __host__ __device__ static inline
#else
#define ESP_HD static inline
#endif

ESP_HD uint32_t esp_ror(uint32_t v, uint32_t n)
{
	return v >> n | v << (32u - n);
}

/* One AES encryption of s (in place) under nr rounds of rk. te0[x] is the
 * column {02, 01, 01, 03} . S[x]; the other three T-tables are byte rotations
 * of it, and S[x] itself is its second byte. */
ESP_HD void esp_aes_encrypt(const uint32_t *rk, uint32_t nr, const uint32_t *te0, uint32_t s[4])
{
	uint32_t s0 = s[0] ^ rk[0], s1 = s[1] ^ rk[1], s2 = s[2] ^ rk[2], s3 = s[3] ^ rk[3];

	for (uint32_t r = 1; r < nr; r++) {
		rk += 4;
		const uint32_t t0 = te0[s0 >> 24] ^ esp_ror(te0[(s1 >> 16) & 0xFFu], 8) ^
				    esp_ror(te0[(s2 >> 8) & 0xFFu], 16) ^ esp_ror(te0[s3 & 0xFFu], 24) ^ rk[0];
		const uint32_t t1 = te0[s1 >> 24] ^ esp_ror(te0[(s2 >> 16) & 0xFFu], 8) ^
				    esp_ror(te0[(s3 >> 8) & 0xFFu], 16) ^ esp_ror(te0[s0 & 0xFFu], 24) ^ rk[1];
		const uint32_t t2 = te0[s2 >> 24] ^ esp_ror(te0[(s3 >> 16) & 0xFFu], 8) ^
				    esp_ror(te0[(s0 >> 8) & 0xFFu], 16) ^ esp_ror(te0[s1 & 0xFFu], 24) ^ rk[2];
		const uint32_t t3 = te0[s3 >> 24] ^ esp_ror(te0[(s0 >> 16) & 0xFFu], 8) ^
				    esp_ror(te0[(s1 >> 8) & 0xFFu], 16) ^ esp_ror(te0[s2 & 0xFFu], 24) ^ rk[3];

		s0 = t0;
		s1 = t1;
		s2 = t2;
		s3 = t3;
	}
	rk += 4;
#define ESP_SB(x) ((te0[(x) & 0xFFu] >> 8) & 0xFFu)
	s[0] = (ESP_SB(s0 >> 24) << 24 | ESP_SB(s1 >> 16) << 16 | ESP_SB(s2 >> 8) << 8 | ESP_SB(s3)) ^ rk[0];
	s[1] = (ESP_SB(s1 >> 24) << 24 | ESP_SB(s2 >> 16) << 16 | ESP_SB(s3 >> 8) << 8 | ESP_SB(s0)) ^ rk[1];
	s[2] = (ESP_SB(s2 >> 24) << 24 | ESP_SB(s3 >> 16) << 16 | ESP_SB(s0 >> 8) << 8 | ESP_SB(s1)) ^ rk[2];
	s[3] = (ESP_SB(s3 >> 24) << 24 | ESP_SB(s0 >> 16) << 16 | ESP_SB(s1 >> 8) << 8 | ESP_SB(s2)) ^ rk[3];
#undef ESP_SB
}

/* z = x . y in GCM's GF(2^128) (SP 800-38D 6.3), bit-serial with both
 * operands in registers: for every bit of x from GCM bit 0 on, z ^= v if it is
 * set, then v = v . x (a right shift, and R = 0xE1 << 120 folded in when a bit
 * falls off). */
ESP_HD void esp_gf_mul(const uint32_t x[4], const uint32_t y[4], uint32_t z[4])
{
	uint32_t v0 = y[0], v1 = y[1], v2 = y[2], v3 = y[3];
	uint32_t z0 = 0, z1 = 0, z2 = 0, z3 = 0;

	for (uint32_t w = 0; w < 4u; w++) {
		uint32_t xw = x[w];

#ifdef __HIP_DEVICE_COMPILE__
#pragma unroll 8
#endif
		for (uint32_t b = 0; b < 32u; b++) {
			const uint32_t m = (uint32_t)((int32_t)xw >> 31);
			const uint32_t r = (0u - (v3 & 1u)) & 0xE1000000u;

			z0 ^= v0 & m;
			z1 ^= v1 & m;
			z2 ^= v2 & m;
			z3 ^= v3 & m;
			v3 = v3 >> 1 | v2 << 31;
			v2 = v2 >> 1 | v1 << 31;
			v1 = v1 >> 1 | v0 << 31;
			v0 = (v0 >> 1) ^ r;
			xw <<= 1;
		}
	}
	z[0] = z0;
	z[1] = z1;
	z[2] = z2;
	z[3] = z3;
}

#ifdef __cplusplus
extern "C" {
#endif
#ifdef __HIPCC__
int odpg_launch_esp(const odpg_esp_args *a, hipStream_t s);
/* words <- 0 with a kernel */
int odpg_launch_esp_clear(uint32_t *p, uint32_t words, hipStream_t s);
#endif
#ifdef __cplusplus
}
#endif

#endif
