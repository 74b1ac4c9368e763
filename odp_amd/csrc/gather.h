/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch interface of the gather kernels (runtime.hip -> gather.hip;
 * include/odpg_gather.h is the public side). Not part of the ABI.
 */
#ifndef ODPG_GATHER_INTERNAL_H_
#define ODPG_GATHER_INTERNAL_H_

#include <stdint.h>
#include "../../include/odpg_gather.h"

#define GTH_TILE ODPG_GATHER_TILE   /* positions per workgroup */

typedef struct odpg_gather_args {
	odpg_gather_src_t src;
	odpg_gather_dst_t dst;
	const uint32_t   *order;
	const uint32_t   *offsets;
	uint32_t          b_first, b_last;
	/* plan workspace, descriptor path only */
	uint64_t         *tsum;   /* [tiles] 16-byte units of a tile, then of the
				   * tiles before it */
	odpg_desc_t      *pos;    /* [max_pkts] source {offset, len} by position */
} odpg_gather_args;

#ifdef __cplusplus
extern "C" {
#endif
#ifdef __HIPCC__
int odpg_launch_gather(const odpg_gather_args *a, hipStream_t s);
#endif
#ifdef __cplusplus
}
#endif

#endif
