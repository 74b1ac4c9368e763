/* SPDX-License-Identifier: BSD-3-Clause
 *
 * odpg_lso.h — large-send offload of a device-resident batch.
 *
 * odp_pktout_send_lso() (platform/linux-generic/odp_packet_io.c:2829-3340)
 * turns one frame into ceil(payload / max_payload) frames, each a copy of the
 * header followed by a slice of the payload, and patches the header of every
 * new frame. odpg_lso() is that job for a whole batch: from a device-resident
 * batch and per-packet (or one uniform) LSO options it writes a dense batch of
 * segments with descriptors, again an ordinary odpg_batch_t / odpg_tx_batch_t,
 * and the host never learns a count. It is the one-to-many stage in front of
 * odpg_tx_prepare(), and the answer to an oversized frame after odpg_l3fwd().
 *
 * Per-packet rules, in the reference's order (_odp_lso_num_packets :3081-3144,
 * _odp_lso_create_packets :3146-3243, lso_update_ipv4 :2977-3010,
 * lso_update_custom :3012-3079). len is the frame length, H = payload_offset,
 * P = max_payload_len:
 *  1. profile >= num_profiles                      -> ODPG_LSO_BAD_PROFILE
 *  2. H > 128 or H > len                           -> ODPG_LSO_BAD_OFFSET
 *  3. H + P > len: one segment, the frame unchanged (:3102-3108); this comes
 *     before every check below
 *  4. IPv4 profile: l3_offset == ODPG_OFFSET_INVALID, H < l3_offset or
 *     H - l3_offset < 20                           -> ODPG_LSO_BAD_L3
 *     otherwise P = P / 8 * 8
 *  5. P == 0 (the reference divides by zero here)  -> ODPG_LSO_BAD_PAYLOAD
 *  6. n = (len - H) / P, left = (len - H) - n * P, n++ if left;
 *     n > 64                                       -> ODPG_LSO_TOO_MANY
 *  7. n == 1: the frame unchanged, no header update (pktout_send_lso
 *     :3256-3262)
 *  8. segment k is bytes [0, H) of the frame followed by bytes
 *     [H + k P, H + k P + P); the last one takes `left` bytes if left != 0.
 *
 * IPv4 profile, per segment of a packet with n > 1 (the header is at
 * l3_offset of the segment):
 *   tot_len = be16((uint16_t)(seglen - l3_offset))
 *   IHL != 5 fails the whole packet                -> ODPG_LSO_BAD_IHL
 *     (lso_update_ipv4 refuses above 5, packet_ipv4_chksum below 5)
 *   frag = (uint16_t)(be16(original frag_offset) + (k * P) / 8): DF, MF and an
 *     original offset are kept, wrap-around is the reference's uint16_t one;
 *     frag |= 0x2000 for k < n - 1
 *   the header checksum as _odp_packet_ipv4_chksum_insert computes it: over
 *     the 20 header bytes with the field zeroed.
 *
 * Custom profile, per segment of a packet with n > 1: the fields in profile
 * order, each a read, modify and write of `size` bytes at `offset` of the
 * segment. A later field sees an earlier field's write; a field may lie in the
 * payload or straddle H. The segment is `first` for k == 0, else `last` for
 * k == n - 1, else `middle`. ODPG_LSO_ADD_SEGMENT_NUM adds k to the big-endian
 * value (size 1: a plain u8 add). ODPG_LSO_WRITE_BITS writes
 * (old & ~mask) | (value & mask). A field whose offset + size exceeds the
 * length of any segment (the last is the shortest) fails the packet with
 * ODPG_LSO_BAD_FIELD, as odp_packet_copy_to_mem does there. num_custom == 0
 * patches nothing.
 *
 * A failed packet has zero segments and its reason in status[i]; packets after
 * it are still segmented. total->first_bad is the smallest failing index (num
 * if none), so the reference's return value and "sent" set are first_bad and
 * positions [0, seg_first[first_bad]), a dense prefix of the output.
 *
 * Layout and capacity are odpg_gather's (odpg_gather.h). Packet i's segments
 * are output positions [seg_first[i], seg_first[i + 1]). Position j starts at
 * the sum of align16(seglen) of the positions before it; padding bytes are
 * zero; dst->desc[j] = {offset, len}. A segment is written whole or not at
 * all: iff its end is <= capacity and j < max_segs. The written segments are a
 * prefix of total->copied segments; the other descriptors below
 * min(num_segs, max_segs) are {0, 0}. Nothing is written at or beyond
 * frames + capacity or desc + max_segs. total->bytes and total->num_segs are
 * always the full need, so they tell what a retry takes. A source frame is
 * read in whole 16-byte units inside [offset, offset + align16(len)).
 *
 * Not covered: the TCP, IPv6 and SCTP protocols (the reference implements
 * none of them) and carrying verdict words or marks over to the segments.
 */
#ifndef ODPG_LSO_H_
#define ODPG_LSO_H_

#include "odpg.h"
#include "odpg_tx.h"   /* ODPG_OFFSET_INVALID */

#ifdef __cplusplus
extern "C" {
#endif

/* odp_lso_protocol_t, odp_lso_modify_t and the PKTIO_LSO_* limits */
#define ODPG_LSO_PROTO_CUSTOM       1u
#define ODPG_LSO_PROTO_IPV4         2u
#define ODPG_LSO_ADD_SEGMENT_NUM    1u
#define ODPG_LSO_WRITE_BITS         5u
#define ODPG_LSO_MAX_CUSTOM         8u
#define ODPG_LSO_MAX_PROFILES       16u
#define ODPG_LSO_MAX_SEGMENTS       64u
#define ODPG_LSO_MAX_PAYLOAD_OFFSET 128u

/* status[i] */
#define ODPG_LSO_OK          0u
#define ODPG_LSO_BAD_PROFILE 1u
#define ODPG_LSO_BAD_OFFSET  2u
#define ODPG_LSO_BAD_L3      3u
#define ODPG_LSO_BAD_PAYLOAD 4u
#define ODPG_LSO_TOO_MANY    5u
#define ODPG_LSO_BAD_IHL     6u
#define ODPG_LSO_BAD_FIELD   7u

/* Packets one workgroup of the copy kernel handles (lso.hip). Informative:
 * batches are of any size; sizes around multiples of it are where the
 * kernels change shape. */
#define ODPG_LSO_TILE 64u

typedef struct odpg_lso_bits_s {   /* odp_lso_write_bits_t, byte 0 */
	uint8_t mask, value;
} odpg_lso_bits_t;

typedef struct odpg_lso_field_s {  /* 12 bytes */
	uint8_t  mod_op;               /* ODPG_LSO_ADD_SEGMENT_NUM / _WRITE_BITS */
	uint8_t  size;                 /* 1, 2, 4 or 8; WRITE_BITS: 1 */
	uint16_t offset;               /* from the start of the segment, <= 128 */
	odpg_lso_bits_t first, middle, last;   /* WRITE_BITS */
	uint16_t reserved;
} odpg_lso_field_t;

typedef struct odpg_lso_profile_s {   /* 104 bytes */
	uint32_t         proto;        /* ODPG_LSO_PROTO_* */
	uint32_t         num_custom;
	odpg_lso_field_t field[ODPG_LSO_MAX_CUSTOM];
} odpg_lso_profile_t;

/* The packet-header fields odp_packet_lso_request() sets, and the L3 offset
 * the IPv4 mode reads. 8 bytes. */
typedef struct odpg_lso_opt_s {
	uint16_t payload_offset;
	uint16_t max_payload_len;
	uint16_t l3_offset;            /* ODPG_OFFSET_INVALID: none */
	uint8_t  profile;              /* index into the plan's profiles */
	uint8_t  reserved;
} odpg_lso_opt_t;

typedef struct odpg_lso_s odpg_lso_t;

typedef struct odpg_lso_src_s {
	const uint8_t        *frames;  /* device */
	const odpg_desc_t    *desc;    /* device, or NULL: fixed stride, len = stride */
	uint32_t              stride;  /* multiple of 16 when desc == NULL */
	uint32_t              num;
	const odpg_lso_opt_t *opt;     /* device, num options, or NULL: `uniform` */
	odpg_lso_opt_t        uniform; /* every packet's options when opt == NULL */
} odpg_lso_src_t;

typedef struct odpg_lso_total_s {  /* device, written by every call */
	uint32_t num_segs;   /* segments of the whole batch */
	uint32_t copied;     /* segments written: the longest prefix that fits */
	uint32_t first_bad;  /* smallest failing packet index, num if none */
	uint32_t reserved;   /* 0 */
	uint64_t bytes;      /* bytes the whole batch needs */
} odpg_lso_total_t;

typedef struct odpg_lso_dst_s {
	uint8_t          *frames;     /* device */
	uint64_t          capacity;   /* bytes writable at frames; <= 2^32 */
	odpg_desc_t      *desc;       /* device, max_segs entries */
	uint32_t          max_segs;
	uint32_t          reserved;
	uint32_t         *seg_first;  /* device, src->num + 1 words */
	uint8_t          *status;     /* device, src->num bytes */
	odpg_lso_total_t *total;      /* device */
} odpg_lso_dst_t;

/* The rules of odp_lso_profile_create (:2836-2885): proto is IPv4 or custom;
 * custom: num_custom <= 8, every field offset <= 128, size 1, 2, 4 or 8,
 * mod_op known, WRITE_BITS only with size 1. Host only, no device needed.
 * 0 or -EINVAL. */
int  odpg_lso_profile_check(const odpg_lso_profile_t *p);

/* Plan: the device workspace for batches of up to max_pkts frames (at most
 * 2^25: 64 segments each stay below 2^32 positions) and a device copy of the
 * profiles. Holds a context reference like counters do (odpg.h "object
 * lifetimes"). -EINVAL for a null argument, num_profiles of 0 or above 16 or
 * a profile odpg_lso_profile_check rejects. */
int  odpg_lso_create(odpg_ctx_t *ctx, const odpg_lso_profile_t *profiles,
		     uint32_t num_profiles, uint32_t max_pkts, odpg_lso_t **plan);
void odpg_lso_destroy(odpg_lso_t *plan);

/* Asynchronous on the context stream; allocates nothing. num == 0 writes
 * seg_first[0] and *total only. -EINVAL, with nothing launched, for a null
 * plan, src, dst, dst->frames, dst->seg_first, dst->status or dst->total
 * (or dst->desc with max_segs != 0, or src->frames with src->num != 0), a
 * frames pointer that is not 16-byte aligned, src->num > max_pkts, a fixed
 * stride that is zero or no multiple of 16, and capacity > 2^32. One call at
 * a time per plan. */
int  odpg_lso(odpg_lso_t *plan, const odpg_lso_src_t *src, const odpg_lso_dst_t *dst);

#ifdef __cplusplus
}
#endif

#endif /* ODPG_LSO_H_ */
