/* SPDX-License-Identifier: BSD-3-Clause
 *
 * odpg_gather.h — dense per-queue frame batches built on the device.
 *
 * _odp_cls_enq() (platform/linux-generic/include/odp_classification_internal.h:
 * 139-225) moves the packets themselves into their queue; odpg_deliver() only
 * moves their indices. odpg_gather() is the move: from a device-resident batch
 * and the delivery lists (`order`, `offsets`) it writes the frames of a range
 * of buckets back to back, in delivery order, with a descriptor array. The
 * result is again an ordinary odpg_batch_t / odpg_fwd_batch_t /
 * odpg_tx_batch_t, so one CoS can be forwarded, classified again with another
 * table or copied to the host without the buckets nobody wants.
 *
 * Positions. The range is read on the device, the host never needs the counts:
 *   e = min(offsets[b_last], src->num), s = min(offsets[b_first], e)
 * and position j in [0, e - s) is source frame i = order[s + j]. `offsets` has
 * at least b_last + 1 words (odpg_deliver wrote B + 1).
 *
 * Layout.
 *   src->desc != NULL  frame j starts at the sum over k < j of
 *                      align16(len[order[s + k]]): every frame starts 16-byte
 *                      aligned, as odpg_desc_t asks. dst->desc[j] = {offset,
 *                      len}. The bytes between len and align16(len) are zero.
 *   src->desc == NULL  frame j starts at j * stride; dst->desc[j] = {j * stride,
 *                      stride} if dst->desc is given.
 *   dst->words[j] = src->words[i] for every position of the range.
 * An order entry >= src->num is never used as an index: it counts as a
 * zero-length frame (descriptors) or yields a zero-filled slot (fixed stride),
 * and its word is 0. Zero-length frames are legal and occupy no bytes.
 *
 * Capacity. A frame is copied whole or not at all: frame j is copied iff its
 * end (offset + align16(len)) is <= dst->capacity. Offsets are monotone, so
 * the copied frames are a prefix of total->copied frames; desc entries of the
 * others are {0, 0}. Nothing is written at or beyond dst->frames + capacity.
 * total->bytes > capacity tells the caller to retry with more room.
 *
 * A source frame is read in whole 16-byte units up to offset + align16(len),
 * the slack every frame buffer of this library already has. src->frames and
 * dst->frames are 16-byte aligned. Marks and odpg_meta_t are not gathered: a
 * caller gathers the verdict words and derives what it needs.
 */
#ifndef ODPG_GATHER_H_
#define ODPG_GATHER_H_

#include "odpg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Positions one workgroup handles (gather.hip). Informative: batches are of
 * any size; sizes around multiples of it are where the kernels change shape. */
#define ODPG_GATHER_TILE 1024u

typedef struct odpg_gather_s odpg_gather_t;

typedef struct odpg_gather_src_s {
	const uint8_t     *frames;  /* device */
	const odpg_desc_t *desc;    /* device, or NULL: fixed stride, len = stride */
	uint32_t           stride;  /* multiple of 16 when desc == NULL */
	uint32_t           num;     /* frames in the source batch */
	const uint32_t    *words;   /* device, num words (e.g. the verdict words), or NULL */
} odpg_gather_src_t;

typedef struct odpg_gather_total_s {  /* device, written by every call */
	uint32_t num;      /* positions in the bucket range */
	uint32_t copied;   /* frames written: the longest prefix that fits capacity */
	uint64_t bytes;    /* bytes the whole range needs */
} odpg_gather_total_t;

typedef struct odpg_gather_dst_s {
	uint8_t             *frames;   /* device */
	uint64_t             capacity; /* bytes writable at frames; <= 2^32 (desc offsets are u32) */
	odpg_desc_t         *desc;     /* device, src->num entries; may be NULL only when src->desc == NULL */
	uint32_t            *words;    /* device, src->num words; required iff src->words */
	odpg_gather_total_t *total;    /* device, required */
} odpg_gather_dst_t;

/* Plan: the device workspace for source batches of up to max_pkts frames.
 * Holds a context reference like counters do (odpg.h "object lifetimes"). */
int  odpg_gather_create(odpg_ctx_t *ctx, uint32_t max_pkts, odpg_gather_t **g);
void odpg_gather_destroy(odpg_gather_t *g);

/* Asynchronous on the context stream, so ordered after the odpg_deliver()
 * launch that wrote the lists; allocates nothing. Buckets [b_first, b_last)
 * are gathered; an empty range writes *dst->total only. -EINVAL, with nothing
 * launched, for a null g, src, order, offsets, dst, dst->frames or
 * dst->total (or src->frames with src->num != 0), a frames pointer that is
 * not 16-byte aligned, src->num > max_pkts, b_first > b_last, capacity > 2^32,
 * a fixed stride that is zero or no multiple of 16, src->desc without
 * dst->desc, and src->words without dst->words or the reverse. One call at a
 * time per plan. */
int  odpg_gather(odpg_gather_t *g, const odpg_gather_src_t *src,
		 const uint32_t *order, const uint32_t *offsets,
		 uint32_t b_first, uint32_t b_last, const odpg_gather_dst_t *dst);

#ifdef __cplusplus
}
#endif

#endif /* ODPG_GATHER_H_ */
