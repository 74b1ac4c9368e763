/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Delivery lists on the device (include/odpg_deliver.h): a stable
 * least-significant-digit-first radix partition of the packet indices by
 * destination bucket, the batch form of _odp_cls_enq() / _odp_cos_enq()
 * (odp_classification_internal.h:139-225).
 *
 * The key is the bucket id, dlv_key_bits(B) bits: one pass up to 11 bits
 * (B <= 2048: every table of the benchmark, C4's B = 1027 included), two
 * passes up to the 18 bits of ODPG_MAX_COS * ODPG_COS_QUEUE_MAX + 2 buckets.
 * The pass kernels, their tile shape and their LDS are in radix_pass.h, which
 * switch.hip shares; here is what makes a verdict word a key.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdint.h>

#include "deliver.h"
#include "radix_pass.h"

namespace {

/* what a pass reads: verdict words (pass 0) or {bucket, index} pairs */
struct Source {
	const uint32_t *src;
	const uint32_t *qbase;
	uint32_t num, num_cos, nq;

	/* include/odpg_deliver.h "Buckets" */
	__device__ __forceinline__ uint32_t key(uint32_t w) const
	{
		const uint32_t c = ODPG_OUT_COS(w);

		if (c < num_cos && !(w & ODPG_OUT_CLS_DROP)) {
			const uint32_t lo = qbase[c], q = ODPG_OUT_HASHQ(w);

			return q < qbase[c + 1u] - lo ? lo + q : nq + 1u;
		}
		return c == ODPG_COS_NOCLS ? nq : nq + 1u;
	}
};

} /* namespace */

extern "C" int odpg_launch_deliver_clear(uint32_t *p, uint32_t words, hipStream_t s)
{
	return rp::clear(p, words, s);
}

extern "C" int odpg_launch_deliver(const odpg_deliver_args *a, hipStream_t s)
{
	const Source src = {a->out, a->qbase, a->num, a->num_cos, a->nbuckets - 2u};
	const rp::Ws ws = {a->order, a->offsets, a->nbuckets, a->key_bits,
			   a->hist, a->dtotal, a->bcount, a->pairs};

	if (!a->num)
		return rp::clear(a->offsets, a->nbuckets + 1u, s);
	return rp::partition(src, ws, s);
}
