/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch interface of the segmentation kernels (runtime.hip -> lso.hip;
 * include/odpg_lso.h is the public side). Not part of the ABI.
 */
#ifndef ODPG_LSO_INTERNAL_H_
#define ODPG_LSO_INTERNAL_H_

#include <stdint.h>
#include "../../include/odpg_lso.h"

#define LSO_TILE ODPG_LSO_TILE   /* packets per workgroup of the copy kernel */

/* what the count pass leaves per packet for the copy pass (16 bytes) */
typedef struct odpg_lso_pk {
	uint32_t off;    /* source descriptor offset (0 with a fixed stride) */
	uint32_t len;
	uint32_t p_l3;   /* effective P | l3_offset << 16 */
	uint32_t hnpf;   /* H | segments << 8 | profile << 16 | LSO_PK_* << 24 */
} odpg_lso_pk;

#define LSO_PK_PATCH 1u   /* segments get header updates */
#define LSO_PK_IPV4  2u

typedef struct odpg_lso_args {
	odpg_lso_src_t src;
	odpg_lso_dst_t dst;
	const odpg_lso_profile_t *profiles;   /* device */
	uint32_t       num_profiles;
	/* plan workspace */
	odpg_lso_pk   *pk;       /* [max_pkts] */
	uint64_t      *tunits;   /* [tiles] 16-byte units of a tile, then of the tiles before it */
	uint32_t      *tsegs;    /* [tiles] segments likewise */
	uint32_t      *tbad;     /* [tiles] smallest failing packet index, ~0 if none */
} odpg_lso_args;

#ifdef __cplusplus
extern "C" {
#endif
#ifdef __HIPCC__
int odpg_launch_lso(const odpg_lso_args *a, hipStream_t s);
#endif
#ifdef __cplusplus
}
#endif

#endif
