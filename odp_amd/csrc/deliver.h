/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch interface of the delivery-list kernels (runtime.hip -> deliver.hip;
 * include/odpg_deliver.h is the public side). Not part of the ABI.
 */
#ifndef ODPG_DELIVER_INTERNAL_H_
#define ODPG_DELIVER_INTERNAL_H_

#include <stdint.h>
#include "../../include/odpg_deliver.h"

#define DLV_TILE       ODPG_DELIVER_TILE   /* packets per workgroup */
#define DLV_DIGIT_BITS 11u                 /* one pass covers B <= 2048 buckets */
#define DLV_RADIX      (1u << DLV_DIGIT_BITS)
/* the largest table has ODPG_MAX_COS * ODPG_COS_QUEUE_MAX + 2 buckets: two
 * digits always cover the bucket id, so one pair buffer is the whole
 * ping-pong workspace */
#define DLV_MAX_BUCKETS (ODPG_MAX_COS * ODPG_COS_QUEUE_MAX + 2u)
#if DLV_MAX_BUCKETS > (1u << (2u * DLV_DIGIT_BITS))
#error "two radix passes must cover every bucket id"
#endif

static inline uint32_t dlv_key_bits(uint32_t nbuckets)
{
	uint32_t b = 1;

	while (b < 32u && (1u << b) < nbuckets)
		b++;
	return b;
}

/* digit width of pass 0 and number of passes for a key of `bits` bits */
static inline uint32_t dlv_bits0(uint32_t bits)
{
	return bits <= DLV_DIGIT_BITS ? bits : (bits + 1u) / 2u;
}

typedef struct odpg_deliver_args {
	const uint32_t *out;      /* verdict words */
	uint32_t        num;
	uint32_t       *order;    /* num packet indices, by bucket */
	uint32_t       *offsets;  /* nbuckets + 1 */
	const uint32_t *qbase;    /* device, num_cos + 1 */
	uint32_t        num_cos;
	uint32_t        nbuckets; /* B */
	uint32_t        key_bits; /* dlv_key_bits(B) */
	uint32_t       *hist;     /* [tiles][digits]: counts, then global bases */
	uint32_t       *dtotal;   /* [DLV_RADIX] digit totals of the running pass
				   * (zero between passes) */
	uint32_t       *bcount;   /* [B] bucket counts, two-pass plans only (zero
				   * between calls) */
	uint32_t       *pairs;    /* num x {bucket, index}, two-pass plans only */
} odpg_deliver_args;

#ifdef __cplusplus
extern "C" {
#endif
#ifdef __HIPCC__
int odpg_launch_deliver(const odpg_deliver_args *a, hipStream_t s);
/* words <- 0 with a kernel (a memset node may not be recorded into a graph) */
int odpg_launch_deliver_clear(uint32_t *p, uint32_t words, hipStream_t s);
#endif
#ifdef __cplusplus
}
#endif

#endif
