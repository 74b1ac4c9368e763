/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch interface of the reassembly kernels (runtime.hip -> reass.hip;
 * include/odpg_reass.h is the public side). Not part of the ABI.
 */
#ifndef ODPG_REASS_INTERNAL_H_
#define ODPG_REASS_INTERNAL_H_

#include <stdint.h>
#include "../../include/odpg_reass.h"

#define REASS_TILE ODPG_REASS_TILE   /* packets per workgroup of the copy kernel */
#define REASS_NONE 0xFFFFFFFFu       /* empty slot, no index, no output */

/* what reass_key leaves per packet (16 bytes) */
typedef struct odpg_reass_pk {
	uint32_t off;    /* source descriptor offset (0 with a fixed stride) */
	uint32_t len;
	uint32_t l_p;    /* L | p << 16 */
	uint32_t hofk;   /* hl | off << 8 | MF << 21 | REASS_K_* << 24 */
} odpg_reass_pk;

#define REASS_K_WHOLE 0u
#define REASS_K_FRAG  1u
#define REASS_K_BAD   3u

/* a group's record, at its leader's index (32 bytes) */
typedef struct odpg_reass_grp {
	unsigned long long sum_p;   /* payload bytes of all members */
	uint32_t nterm;             /* members with MF == 0 */
	uint32_t W;                 /* largest end of such a member */
	uint32_t first;             /* smallest index of a member with off == 0 */
	uint32_t last;              /* largest member index */
	uint32_t miss;              /* a member with MF == 1 has no successor */
	uint32_t base;              /* 16-byte unit the output starts at, REASS_NONE: not written */
} odpg_reass_grp;

typedef struct odpg_reass_args {
	odpg_reass_src_t src;
	odpg_reass_dst_t dst;
	/* plan workspace */
	odpg_reass_pk  *pk;      /* [max_pkts] */
	odpg_reass_grp *grp;     /* [max_pkts] */
	uint32_t       *lead;    /* [max_pkts] a fragment's group */
	uint32_t       *obase;   /* [max_pkts] output length, then the unit a WHOLE frame goes to */
	uint32_t       *flow;    /* [tsize] flow table: the leader's index */
	unsigned long long *pos; /* [tsize] (leader, start byte) of every fragment */
	uint32_t        tsize;   /* of this call: a power of two >= 2 num */
	uint32_t        reserved;
	uint64_t       *tunits;  /* [tiles] 16-byte units of a tile, then of the tiles before it */
	uint32_t       *touts;   /* [tiles] outputs likewise */
	uint32_t       *theld;   /* [tiles] held fragments likewise */
	uint32_t       *tbad;    /* [tiles] BAD fragments */
} odpg_reass_args;

#ifdef __cplusplus
extern "C" {
#endif
#ifdef __HIPCC__
int odpg_launch_reass(const odpg_reass_args *a, hipStream_t s);
#endif
#ifdef __cplusplus
}
#endif

#endif
