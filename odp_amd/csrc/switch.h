/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch interface of the L2 switch kernels (runtime.hip -> switch.hip;
 * include/odpg_switch.h is the public side). Not part of the ABI.
 */
#ifndef ODPG_SWITCH_INTERNAL_H_
#define ODPG_SWITCH_INTERNAL_H_

#include <stdint.h>
#include "../../include/odpg_switch.h"
#include "deliver.h"   /* the radix partition's tile and digit widths */

#define SW_TILE    ODPG_SWITCH_TILE          /* packets per resolve / list workgroup */
#define SW_SLOTS   ODPG_SWITCH_TABLE_SIZE
/* partition keys: a learning packet's source slot, SW_SLOTS for a dropped one */
#define SW_BUCKETS (SW_SLOTS + 1u)
#define SW_KEY_BITS 17u
/* tile counts, a column per port, then the fields of odpg_switch_total_t:
 * unicast, flooded, dropped, entries */
#define SW_COL_KIND    ODPG_SWITCH_MAX_PORTS
#define SW_COL_ENTRIES (SW_COL_KIND + 3u)
#define SW_COLS        (SW_COL_KIND + 4u)

/* what sw_key leaves per packet (16 bytes) */
typedef struct odpg_switch_rec {
	uint32_t dst_lo;   /* dst bytes 0-3 */
	uint32_t dst_src;  /* dst bytes 4-5 | src bytes 0-1 << 16 */
	uint32_t src_hi;   /* src bytes 2-5 */
	uint32_t meta;     /* port_in | kind << 8 | dst slot << 16 */
} odpg_switch_rec;

/* kind of a record: to be resolved, or an ODPG_SWITCH_DROP_* */
#define SW_K_FWD 0u

typedef struct odpg_switch_args {
	odpg_switch_src_t src;
	odpg_switch_dst_t dst;
	uint32_t num_ports;
	uint32_t cur_tick;
	uint64_t *table;          /* [SW_SLOTS] */
	/* plan workspace */
	odpg_switch_rec *rec;     /* [max_pkts] */
	uint32_t *skey;           /* [max_pkts] partition keys */
	uint32_t *mask;           /* [max_pkts] ports a packet goes to */
	uint32_t *order;          /* [max_pkts] indices by key: slot s's writers ascending */
	uint32_t *offsets;        /* [SW_BUCKETS + 1] */
	uint32_t *tcnt;           /* [SW_COLS][tiles of the call] counts, then list bases */
	uint32_t *hist, *dtotal, *bcount, *pairs;   /* radix_pass.h */
} odpg_switch_args;

#ifdef __cplusplus
extern "C" {
#endif
#ifdef __HIPCC__
int odpg_launch_switch(const odpg_switch_args *a, hipStream_t s);
/* words <- 0 with a kernel */
int odpg_launch_switch_clear(uint32_t *p, uint32_t words, hipStream_t s);
#endif
#ifdef __cplusplus
}
#endif

#endif
