/* SPDX-License-Identifier: BSD-3-Clause
 *
 * odpg_reass.h — IPv4 reassembly of a device-resident batch.
 *
 * The many-to-one counterpart of odpg_lso(): every datagram whose fragments
 * are all inside the batch becomes one frame again, frames that are no
 * fragments pass unchanged, and the fragments of datagrams that are not
 * complete yet are reported as a `held` list the caller carries into the next
 * batch with odpg_gather(). The reference's example/ipfragreass keeps
 * per-bucket lists with timestamps and a garbage collector; this batch form is
 * stateless and deterministic, timeouts stay with the caller. Kept from it:
 * the flow key (equal_flow, odp_ipfragreass_reassemble.c:26-36), what a
 * complete chain is (extract_complete_packet :168-281) and how the result's
 * header is fixed (send_packet :325-333).
 *
 * Per-packet rules. fr is the frame, n its length, L its L3 offset; fields
 * are big-endian.
 *  1. WHOLE (status 0) if L == ODPG_OFFSET_INVALID, L + 20 > n, the version
 *     nibble is not 4, IHL < 5 or L + 4 IHL > n.
 *  2. f = be16(fr[L + 6]), MF = f & 0x2000, off = f & 0x1FFF. MF == 0 and
 *     off == 0: WHOLE. A WHOLE packet is an output frame, copied unchanged.
 *  3. Otherwise a fragment: hl = 4 IHL, tl = be16(tot_len), p = tl - hl. BAD
 *     (status 3) if p <= 0, L + tl > n, or MF is set and p % 8 != 0. A BAD
 *     fragment is dropped: no output, not held, counted in num_bad. Frame
 *     bytes beyond L + tl (padding) are never copied.
 *  4. The flow is src, dst (fr[L + 12 .. L + 20)), id (fr[L + 4 .. L + 6)) and
 *     proto (fr[L + 9]). A group is every non-BAD fragment of the batch with
 *     equal flow; L, hl and the L2 bytes are not part of the key.
 *  5. A group is complete iff its members, ordered by off, tile [0, W)
 *     exactly (the first has off == 0, each next one starts at 8 off where
 *     the previous one ended at 8 off + p, the last is the only member with
 *     MF == 0 and W is its end) and hl0 + W <= 65535, member 0 being the
 *     off == 0 member. Duplicates, overlaps, holes, two terminals or a missing
 *     first fragment make a group incomplete. Up to 8191 members.
 *  6. A complete group yields one frame: fr0[0, L0 + hl0) followed by every
 *     member's payload in offset order; at L0 tot_len = hl0 + W, the fragment
 *     field is f0 & 0xC000 (DF and the reserved bit kept) and the header
 *     checksum is computed over the hl0 bytes with the field zeroed. Members
 *     get status JOINED (1), members of incomplete groups HELD (2).
 *  7. Every output has an emitting index: a WHOLE packet's own index, a
 *     group's largest member index (the arrival that completes it). Outputs
 *     are in ascending emitting index. origin[j] is the WHOLE packet's index
 *     or the index of member 0: the frame whose L2 and IP header the output
 *     carries. It is written for every j < min(num_out, max_out).
 *  8. held[0, num_held) are the HELD indices in ascending order and
 *     held_offsets = {0, num_held}: a one-bucket delivery list for
 *     odpg_gather(..., held, held_offsets, 0, 1, ...).
 *
 * Layout and capacity are odpg_gather's and odpg_lso's. Position j starts at
 * the sum of align16(len) of the positions before it; padding is zero. A frame
 * is written whole or not at all: iff its end is <= capacity and j < max_out.
 * The written frames are a prefix of total->copied frames; the other
 * descriptors below min(num_out, max_out) are {0, 0}. total->bytes and
 * total->num_out are always the full need. Nothing is written at or beyond
 * frames + capacity, desc + max_out or origin + max_out. A source frame is
 * read in whole 16-byte units inside [offset, offset + align16(len)); a
 * hostile l3_offset or tot_len never indexes outside that.
 *
 * Every output is byte-identical from run to run. Not covered: state across
 * batches, IPv6 fragment headers, overlap resolution, carrying verdict words
 * or marks (origin is the hook for that).
 */
#ifndef ODPG_REASS_H_
#define ODPG_REASS_H_

#include "odpg.h"
#include "odpg_tx.h"   /* ODPG_OFFSET_INVALID */

#ifdef __cplusplus
extern "C" {
#endif

/* status[i] */
#define ODPG_REASS_WHOLE  0u
#define ODPG_REASS_JOINED 1u
#define ODPG_REASS_HELD   2u
#define ODPG_REASS_BAD    3u

/* Packets one workgroup of the copy kernel handles (reass.hip). Informative:
 * batches are of any size; sizes around multiples of it are where the
 * kernels change shape. */
#define ODPG_REASS_TILE 64u

typedef struct odpg_reass_s odpg_reass_t;

typedef struct odpg_reass_src_s {
	const uint8_t     *frames;     /* device */
	const odpg_desc_t *desc;       /* device, or NULL: fixed stride, len = stride */
	uint32_t           stride;     /* multiple of 16 when desc == NULL */
	uint32_t           num;
	const void        *l3_offset;  /* device: u16 entries l3_stride bytes apart, or NULL */
	uint32_t           l3_stride;  /* even, >= 2 (2: a dense array; sizeof(odpg_meta_t):
					* &meta[0].l3_offset of a classify result) */
	uint16_t           uniform_l3; /* every packet's L3 offset when l3_offset == NULL */
	uint16_t           reserved;
} odpg_reass_src_t;

typedef struct odpg_reass_total_s {  /* device, written by every call */
	uint32_t num_out;   /* output frames of the whole batch */
	uint32_t copied;    /* frames written: the longest prefix that fits */
	uint32_t num_held;
	uint32_t num_bad;
	uint64_t bytes;     /* bytes the whole output needs */
} odpg_reass_total_t;

typedef struct odpg_reass_dst_s {
	uint8_t            *frames;       /* device */
	uint64_t            capacity;     /* bytes writable at frames; <= 2^32 */
	odpg_desc_t        *desc;         /* device, max_out entries */
	uint32_t            max_out;
	uint32_t            reserved;
	uint32_t           *origin;       /* device, max_out words */
	uint8_t            *status;       /* device, src->num bytes */
	uint32_t           *held;         /* device, src->num words */
	uint32_t           *held_offsets; /* device, 2 words */
	odpg_reass_total_t *total;        /* device */
} odpg_reass_dst_t;

/* Plan: the device workspace (per-packet records, group records and the two
 * hash tables) for batches of up to max_pkts frames, at most 2^24. Holds a
 * context reference like counters do (odpg.h "object lifetimes"). */
int  odpg_reass_create(odpg_ctx_t *ctx, uint32_t max_pkts, odpg_reass_t **plan);
void odpg_reass_destroy(odpg_reass_t *plan);

/* Asynchronous on the context stream; allocates nothing; no host sync.
 * num == 0 writes *total and held_offsets only. -EINVAL, with nothing
 * launched, for a null plan, src, dst, dst->frames, dst->status, dst->held,
 * dst->held_offsets or dst->total (or dst->desc / dst->origin with
 * max_out != 0, or src->frames with src->num != 0), a frames pointer that is
 * not 16-byte aligned, src->num > max_pkts, a fixed stride that is zero or no
 * multiple of 16, an l3_offset array with an odd address or an odd or zero
 * l3_stride, and capacity > 2^32. One call at a time per plan. */
int  odpg_reass(odpg_reass_t *plan, const odpg_reass_src_t *src, const odpg_reass_dst_t *dst);

#ifdef __cplusplus
}
#endif

#endif /* ODPG_REASS_H_ */
