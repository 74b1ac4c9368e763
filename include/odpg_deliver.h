/* SPDX-License-Identifier: BSD-3-Clause
 *
 * odpg_deliver.h — device-side CoS queue delivery lists.
 *
 * The device form of _odp_cls_enq() / _odp_cos_enq()
 * (platform/linux-generic/include/odp_classification_internal.h:139-225) for
 * a device-resident batch: from the verdict words odpg_classify() wrote, one
 * call produces, per destination queue, the packet indices delivered to it in
 * arrival order. The reference enqueues run-length batches in arrival order,
 * so every queue sees its packets in arrival order; a stable partition of the
 * packet indices by destination is exactly that per-queue order.
 *
 * Buckets of a table with num_cos CoS: CoS c has nq[c] = max(num_queue, 1)
 * queues, qbase[c] is the exclusive prefix sum of nq (the queue columns of
 * the sharded counters, odpg.h) and NQ = qbase[num_cos]. A verdict word w
 * belongs to
 *   qbase[c] + ODPG_OUT_HASHQ(w)   c = ODPG_OUT_COS(w) < num_cos,
 *                                  ODPG_OUT_CLS_DROP clear and
 *                                  ODPG_OUT_HASHQ(w) < nq[c]: delivered to
 *                                  that queue of CoS c
 *   NQ      ODPG_DELIVER_PKTIN     ODPG_OUT_COS(w) == ODPG_COS_NOCLS: the
 *                                  classifier is disabled, the packet goes to
 *                                  the pktin queue / out[]
 *   NQ + 1  ODPG_DELIVER_FREE      everything else: ODPG_COS_NONE / PDROP /
 *                                  LOOP, a drop-action CoS, and any word that
 *                                  names no queue of the table
 * B = NQ + 2 buckets in all.
 */
#ifndef ODPG_DELIVER_H_
#define ODPG_DELIVER_H_

#include "odpg.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the last two buckets of a plan with B = odpg_deliver_num_buckets() */
#define ODPG_DELIVER_PKTIN(B) ((uint32_t)(B) - 2u)
#define ODPG_DELIVER_FREE(B)  ((uint32_t)(B) - 1u)

/* Packets one workgroup ranks (deliver.hip). Informative: batches are of any
 * size; sizes around multiples of it are where the kernels change shape. */
#define ODPG_DELIVER_TILE 4096u

typedef struct odpg_deliver_s odpg_deliver_t;

/* Plan: the bucket layout of `tbl` and the device workspace for batches of up
 * to max_pkts packets. Holds a context reference like counters do (odpg.h
 * "object lifetimes"). */
int      odpg_deliver_create(odpg_ctx_t *ctx, const odpg_table_t *tbl, uint32_t max_pkts,
			     odpg_deliver_t **d);
void     odpg_deliver_destroy(odpg_deliver_t *d);
uint32_t odpg_deliver_num_buckets(const odpg_deliver_t *d);
/* qbase[cos]; < 0 if cos >= num_cos */
int      odpg_deliver_queue_base(const odpg_deliver_t *d, uint32_t cos);
/* 1 if the plan serves `tbl` (same CoS count and queue counts), else 0 */
int      odpg_deliver_match(const odpg_deliver_t *d, const odpg_table_t *tbl);

/* Asynchronous on the context stream, so ordered after the odpg_classify()
 * launch that wrote `out`; allocates nothing. out: device, num words. order:
 * device, num words. offsets: device, B + 1 words. Afterwards
 * order[offsets[b] .. offsets[b + 1]) holds exactly the indices i whose word
 * out[i] belongs to bucket b, strictly ascending; offsets[0] == 0 and
 * offsets[B] == num. num == 0 writes offsets only. -EINVAL for a null pointer
 * or num > max_pkts. One call at a time per plan. */
int      odpg_deliver(odpg_deliver_t *d, const odpg_out_t *out, uint32_t num,
		      uint32_t *order, uint32_t *offsets);

#ifdef __cplusplus
}
#endif

#endif /* ODPG_DELIVER_H_ */
