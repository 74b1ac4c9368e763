/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Host runtime behind the odpg.h C-ABI: contexts (device + stream + scratch),
 * compiled rule tables in HBM, device-resident and host-buffer batch
 * classification, and thin memory / timing helpers.
 */
#include <hip/hip_runtime.h>
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <vector>

#include "../../include/odpg.h"
#include "odpg_internal.h"
#include "stats_commit.h"
#include "cls_compile.h"
#include "deliver.h"
#include "gather.h"
#include "lso.h"
#include "reass.h"
#include "switch.h"
#include "esp.h"
#include "lanes.h"


extern "C" int odpg_launch_classify(const odpg_launch_args *a, hipStream_t s);
extern "C" uint32_t odpg_launch_grid(uint32_t num);

#define NUM_EVENTS 16

/* host-path staging (odpg_classify_host): NSTAGE buffer sets cycle
 * through H2D (copy stream) -> classify + D2H (context stream); kept in the
 * context and grown on demand, so repeated calls allocate nothing */
#define NSTAGE 3

struct Stage {
	uint8_t *frames;
	odpg_desc_t *desc;
	odpg_out_t *out;
	uint16_t *mark;
	odpg_meta_t *meta;
	odpg_desc_t *hdesc;    /* pinned host, chunk-relative descriptors */
	hipEvent_t h2d_done, compute_done;
};

struct odpg_ctx_s {
	int device;
	hipStream_t stream;
	bool own_stream;
	hipStream_t copy_stream;
	/* launch lanes (lanes.h): lane 0 is `stream`, lane 1 `lane1`; verdict-only
	 * launches and launches counted into per-lane rows alternate between them,
	 * every other use of the context stream goes through ctx_stream() /
	 * ctx_stream_locked(), which join first */
	hipStream_t lane1;
	hipEvent_t lane_ev[2][LANE_NEV];
	lane_state ls;
	bool handed_out;   /* odpg_ctx_stream() gave the raw stream away: one lane for good */
	void *ws;          /* per-workgroup counter partials */
	uint64_t *sred;    /* stats_commit scratch (SRED_BYTES, kept zeroed) */
	Stage stage[NSTAGE];
	size_t stage_span;     /* bytes of frames per stage */
	uint32_t stage_chunk;  /* packets per stage (out / desc / mark / meta) */
	uint32_t stage_flags;  /* 1 desc, 2 mark, 4 meta allocated */
	uint64_t *stage_stats;
	uint32_t stage_nstats;
	size_t ws_bytes;
	hipEvent_t ev[NUM_EVENTS];
	int kernel_mode;   /* 0 auto, 1 walk, 2 evaluate-all, 3 hash walk */
	std::mutex lock;
	/* the caller's handle + one per counters / forwarder / fence created on
	 * the context (odpg.h "object lifetimes"): the stream and device memory
	 * are freed when the last of them is released */
	std::atomic<int> refs;
};

static void free_stage(odpg_ctx_t *c);

struct odpg_table_s {
	dtable_hdr_t hdr;
	std::vector<uint8_t> blob;
	void *dblob;
	int device;
	int cycle;
	uint32_t depth;    /* longest rule chain from the default CoS (0: a cycle) */
	uint64_t qsig;     /* counter layout: CoS count, queues and stats flags */
	size_t cap;        /* bytes allocated at dblob */
	hipEvent_t uploaded;   /* the last upload of `blob` has been consumed */
};

/* odpg.h "sharded counters" */
struct odpg_counters_s {
	odpg_ctx_t *ctx;
	uint64_t qsig;
	uint32_t ncos, ncols, words, rows;
	uint32_t sets;                 /* row sets: one per launch lane, or 1 (launches stay serial) */
	uint32_t any_cos;              /* some CoS has stats_enable */
	uint64_t *drows;               /* device, sets x rows x words */
	uint32_t *dqcol;               /* device, queue column of each CoS */
	uint64_t *dsum;                /* device, words (fold target) */
	uint64_t *hsum;                /* pinned host, words */
	hipEvent_t done;
	std::vector<uint32_t> qcol;    /* host: ncos + 1 prefix of num_queue */
	std::vector<uint8_t> nq;
	std::mutex lock;               /* one fold at a time */
};

/* The longest chain of rules cls_select_cos can follow from the default CoS
 * (odp_classification.c:1599-1631: at CoS c every rule of c may lead to its
 * destination, whose rules are tried next), or 0 when a cycle is reachable.
 * The lean kernel walks exactly that many levels, without a loop. */
static uint32_t table_walk_depth(const odpg_table_t *t)
{
	const dtable_hdr_t &h = t->hdr;
	const dcos_t *hc = (const dcos_t *)(t->blob.data() + h.cos_off);
	const uint32_t *pinfo = (const uint32_t *)(t->blob.data() + h.pinfo_off);
	const int32_t dc = h.default_cos;

	if (dc < 0 || (uint32_t)dc >= h.num_cos || !hc[dc].valid)
		return 1;
	std::vector<uint8_t> state(h.num_cos, 0);     /* 0 new, 1 on path, 2 done */
	std::vector<uint32_t> len(h.num_cos, 0);
	bool cyclic = false;
	/* iterative DFS: longest number of rules from c */
	std::vector<std::pair<uint32_t, uint32_t>> st{{(uint32_t)dc, 0u}};

	state[dc] = 1;
	while (!st.empty() && !cyclic) {
		auto &[c, i] = st.back();

		if (i < hc[c].nrule) {
			const uint32_t k = hc[c].rule_start + i++;
			const uint32_t d = k < h.num_pmr ? (pinfo[k] & 0xffffu) : 0xffffu;

			if (d >= h.num_cos)
				continue;
			if (state[d] == 1) {
				cyclic = true;
			} else if (state[d] == 0) {
				state[d] = 1;
				st.push_back({d, 0u});
			}
		} else {
			uint32_t best = 0;

			for (uint32_t r = 0; r < hc[c].nrule; r++) {
				const uint32_t k = hc[c].rule_start + r;
				const uint32_t d = k < h.num_pmr ? (pinfo[k] & 0xffffu) : 0xffffu;

				if (d < h.num_cos)
					best = std::max(best, 1u + len[d]);
			}
			len[c] = best;
			state[c] = 2;
			st.pop_back();
		}
	}
	return cyclic ? 0u : std::max(len[dc], 1u);
}

/* layout signature of a table's counters: a counters object serves every
 * table with the same CoS count, queue counts and stats flags */
static uint64_t table_qsig(const odpg_table_t *t)
{
	const dcos_t *hc = (const dcos_t *)(t->blob.data() + t->hdr.cos_off);
	uint64_t h = 1469598103934665603ull ^ t->hdr.num_cos;

	for (uint32_t c = 0; c < t->hdr.num_cos; c++) {
		const uint32_t nq = hc[c].num_queue ? hc[c].num_queue : 1u;

		h = (h ^ (nq | ((uint32_t)(hc[c].stats != 0) << 8))) * 1099511628211ull;
	}
	return h;
}

/* the events and stream waits lanes.h decided, in order */
static int lane_apply(odpg_ctx_t *c, const lane_act *acts, int n)
{
	for (int i = 0; i < n; i++) {
		const lane_act &a = acts[i];
		hipStream_t own = a.lane ? c->lane1 : c->stream;
		hipStream_t other = a.lane ? c->stream : c->lane1;
		hipEvent_t e = c->lane_ev[a.lane][a.slot];
		const hipError_t rc = a.op == LANE_RECORD ? hipEventRecord(e, own)
							  : hipStreamWaitEvent(other, e, 0);

		if (rc != hipSuccess) {
			fprintf(stderr, "odpg: lane %s failed: %s\n",
				a.op == LANE_RECORD ? "event record" : "stream wait",
				hipGetErrorString(rc));
			return -EIO;
		}
	}
	return 0;
}

/* The context stream for anything but a launch on the lanes: ordered after
 * every launch already enqueued on either lane (c->lock held). */
static hipStream_t ctx_stream_locked(odpg_ctx_t *c)
{
	if (c->lane1) {
		lane_act acts[LANE_MAX_ACTS];
		int n;

		lane_join(&c->ls, acts, &n);
		lane_apply(c, acts, n);
	}
	return c->stream;
}

static hipStream_t ctx_stream(odpg_ctx_t *c)
{
	std::lock_guard<std::mutex> g(c->lock);

	return ctx_stream_locked(c);
}

#define HIPCHK(x)                                                              \
	do {                                                                   \
		hipError_t e_ = (x);                                           \
		if (e_ != hipSuccess) {                                        \
			fprintf(stderr, "odpg: %s failed: %s (%s:%d)\n", #x,    \
				hipGetErrorString(e_), __FILE__, __LINE__);    \
			return -EIO;                                           \
		}                                                              \
	} while (0)

extern "C" {

int odpg_abi_version(void)
{
	return ODPG_ABI_VERSION;
}

const char *odpg_build_info(void)
{
	return "odpg gfx950 classifier, ABI 2";
}

int odpg_device_count(void)
{
	int n = 0;

	if (hipGetDeviceCount(&n) != hipSuccess)
		return 0;
	return n;
}

int odpg_ctx_create(int device, void *stream, odpg_ctx_t **out)
{
	if (!out)
		return -EINVAL;
	int n = odpg_device_count();

	if (device < 0 || device >= n)
		return -ENODEV;
	odpg_ctx_t *c = new odpg_ctx_t();

	c->device = device;
	c->ws = nullptr;
	c->ws_bytes = 0;
	c->kernel_mode = 0;
	c->lane1 = nullptr;
	c->handed_out = false;
	lane_init(&c->ls, 1);
	c->refs.store(1);
	if (hipSetDevice(device) != hipSuccess) {
		delete c;
		return -EIO;
	}
	if (stream) {
		c->stream = (hipStream_t)stream;
		c->own_stream = false;
	} else {
		if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) {
			delete c;
			return -EIO;
		}
		c->own_stream = true;
		/* the second lane: with the copy stream, three streams a context */
		if (hipStreamCreateWithFlags(&c->lane1, hipStreamNonBlocking) != hipSuccess) {
			hipStreamDestroy(c->stream);
			delete c;
			return -EIO;
		}
		for (int l = 0; l < 2; l++)
			for (int k = 0; k < LANE_NEV; k++)
				if (hipEventCreateWithFlags(&c->lane_ev[l][k], hipEventDisableTiming) != hipSuccess) {
					delete c;
					return -EIO;
				}
		lane_init(&c->ls, 2);
	}
	if (hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking) != hipSuccess) {
		delete c;
		return -EIO;
	}
	for (int k = 0; k < NUM_EVENTS; k++)
		if (hipEventCreate(&c->ev[k]) != hipSuccess) {
			delete c;
			return -EIO;
		}
	if (hipMalloc(&c->sred, SRED_BYTES) != hipSuccess ||
	    hipMemset(c->sred, 0, SRED_BYTES) != hipSuccess) {
		delete c;
		return -EIO;
	}
	for (int k = 0; k < NSTAGE; k++)
		if (hipEventCreateWithFlags(&c->stage[k].h2d_done, hipEventDisableTiming) != hipSuccess ||
		    hipEventCreateWithFlags(&c->stage[k].compute_done, hipEventDisableTiming) != hipSuccess) {
			delete c;
			return -EIO;
		}
	*out = c;
	return 0;
}

/* the context's resources, once nothing refers to it any more */
static void ctx_free(odpg_ctx_t *c)
{
	hipSetDevice(c->device);
	hipStreamSynchronize(c->stream);
	if (c->lane1)
		hipStreamSynchronize(c->lane1);
	hipStreamSynchronize(c->copy_stream);
	if (c->ws)
		hipFree(c->ws);
	hipFree(c->sred);
	free_stage(c);
	hipFree(c->stage_stats);
	for (int k = 0; k < NSTAGE; k++) {
		hipEventDestroy(c->stage[k].h2d_done);
		hipEventDestroy(c->stage[k].compute_done);
	}
	for (int k = 0; k < NUM_EVENTS; k++)
		hipEventDestroy(c->ev[k]);
	hipStreamDestroy(c->copy_stream);
	if (c->lane1) {
		for (int l = 0; l < 2; l++)
			for (int k = 0; k < LANE_NEV; k++)
				hipEventDestroy(c->lane_ev[l][k]);
		hipStreamDestroy(c->lane1);
	}
	if (c->own_stream)
		hipStreamDestroy(c->stream);
	delete c;
}

void odpg_ctx_ref(odpg_ctx_t *c)
{
	c->refs.fetch_add(1);
}

void odpg_ctx_unref(odpg_ctx_t *c)
{
	if (c->refs.fetch_sub(1) == 1)
		ctx_free(c);
}

void odpg_ctx_destroy(odpg_ctx_t *c)
{
	if (!c)
		return;
	/* the odp_cls bindings on this context go now (their counters and
	 * tables); objects the caller still holds keep the context alive */
	odpg_cls_ctx_release(c);
	odpg_ctx_unref(c);
}

int odpg_ctx_set_kernel_mode(odpg_ctx_t *c, int mode)
{
	if (!c || mode < 0 || mode > 3)
		return -EINVAL;
	c->kernel_mode = mode;
	return 0;
}

void *odpg_ctx_stream(odpg_ctx_t *c)
{
	if (!c)
		return nullptr;
	/* the caller may enqueue work the library cannot see: one lane from here on */
	std::lock_guard<std::mutex> g(c->lock);

	if (c->lane1) {
		lane_act acts[LANE_MAX_ACTS];
		int n;

		lane_set(&c->ls, 1, acts, &n);
		lane_apply(c, acts, n);
	}
	c->handed_out = true;
	return (void *)c->stream;
}

/* fwd.hip, tx.hip, diag.hip: the context stream, joined, lanes kept */
void *odpg_ctx_stream_joined(odpg_ctx_t *c)
{
	return (void *)ctx_stream(c);
}

int odpg_ctx_lanes(odpg_ctx_t *c)
{
	if (!c)
		return -EINVAL;
	std::lock_guard<std::mutex> g(c->lock);

	return c->ls.lanes;
}

int odpg_ctx_set_lanes(odpg_ctx_t *c, int lanes)
{
	if (!c || (lanes != 1 && lanes != 2))
		return -EINVAL;
	std::lock_guard<std::mutex> g(c->lock);

	if (lanes == c->ls.lanes)
		return 0;
	if (lanes == 2 && (!c->lane1 || c->handed_out))
		return -EPERM;   /* a caller's stream, or the stream was handed out */
	lane_act acts[LANE_MAX_ACTS];
	int n;

	lane_set(&c->ls, lanes, acts, &n);
	return lane_apply(c, acts, n);
}

int odpg_ctx_sync(odpg_ctx_t *c)
{
	if (!c)
		return -EINVAL;
	HIPCHK(hipStreamSynchronize(ctx_stream(c)));
	return 0;
}

/* compiled-table image: this header, dtable_hdr_t, then the blob */
struct table_image_hdr {
	uint32_t magic;        /* IMAGE_MAGIC */
	uint32_t abi;          /* ODPG_ABI_VERSION */
	uint32_t hdr_bytes;    /* sizeof(dtable_hdr_t) */
	uint32_t blob_bytes;
};
#define IMAGE_MAGIC 0x5450444fu   /* "ODPT" in memory order */

int odpg_rules_compile(const odpg_rules_t *rules, void *image, size_t *size)
{
	if (!rules || !size)
		return -EINVAL;
	std::vector<uint8_t> blob;
	dtable_hdr_t hdr;
	int rc = odpg_compile_rules(rules, blob, &hdr);

	if (rc)
		return rc;
	const size_t need = sizeof(table_image_hdr) + sizeof(dtable_hdr_t) + hdr.blob_bytes;

	if (!image || *size < need) {
		*size = need;
		return -ENOSPC;
	}
	table_image_hdr ih = {IMAGE_MAGIC, ODPG_ABI_VERSION, (uint32_t)sizeof(dtable_hdr_t),
			      hdr.blob_bytes};
	uint8_t *o = (uint8_t *)image;

	memcpy(o, &ih, sizeof(ih));
	memcpy(o + sizeof(ih), &hdr, sizeof(hdr));
	memcpy(o + sizeof(ih) + sizeof(hdr), blob.data(), hdr.blob_bytes);
	*size = need;
	return 0;
}

/* a compiled table (host blob + header) onto the context's device */
static int table_upload(odpg_ctx_t *c, odpg_table_t *t, odpg_table_t **out)
{
	t->cycle = odpg_rules_has_cycle(t->blob, t->hdr);
	t->depth = table_walk_depth(t);
	t->device = c->device;
	t->qsig = table_qsig(t);
	t->uploaded = nullptr;
	hipSetDevice(c->device);
	if (hipMalloc(&t->dblob, t->hdr.blob_bytes) != hipSuccess) {
		delete t;
		return -ENOMEM;
	}
	t->cap = t->hdr.blob_bytes;
	hipStream_t cs = ctx_stream(c);

	if (hipMemcpyAsync(t->dblob, t->blob.data(), t->hdr.blob_bytes, hipMemcpyHostToDevice,
			   cs) != hipSuccess ||
	    hipStreamSynchronize(cs) != hipSuccess) {
		hipFree(t->dblob);
		delete t;
		return -EIO;
	}
	*out = t;
	return 0;
}

int odpg_table_import(odpg_ctx_t *c, const void *image, size_t size, odpg_table_t **out)
{
	if (!c || !image || !out || size < sizeof(table_image_hdr))
		return -EINVAL;
	table_image_hdr ih;

	memcpy(&ih, image, sizeof(ih));
	if (ih.magic != IMAGE_MAGIC || ih.abi != ODPG_ABI_VERSION ||
	    ih.hdr_bytes != sizeof(dtable_hdr_t) ||
	    size != sizeof(ih) + sizeof(dtable_hdr_t) + (size_t)ih.blob_bytes)
		return -EINVAL;
	odpg_table_t *t = new odpg_table_t();

	memcpy(&t->hdr, (const uint8_t *)image + sizeof(ih), sizeof(dtable_hdr_t));
	if (t->hdr.blob_bytes != ih.blob_bytes) {
		delete t;
		return -EINVAL;
	}
	t->blob.assign((const uint8_t *)image + sizeof(ih) + sizeof(dtable_hdr_t),
		       (const uint8_t *)image + size);
	return table_upload(c, t, out);
}

int odpg_table_create(odpg_ctx_t *c, const odpg_rules_t *rules, odpg_table_t **out)
{
	if (!c || !rules || !out)
		return -EINVAL;
	odpg_table_t *t = new odpg_table_t();
	int rc = odpg_compile_rules(rules, t->blob, &t->hdr);

	if (rc) {
		delete t;
		return rc;
	}
	return table_upload(c, t, out);
}

int odpg_table_update(odpg_ctx_t *c, odpg_table_t *t, const odpg_rules_t *rules)
{
	if (!c || !t || !rules)
		return -EINVAL;
	if (t->device != c->device)
		return -EXDEV;
	std::vector<uint8_t> blob;
	dtable_hdr_t hdr;
	int rc = odpg_compile_rules(rules, blob, &hdr);

	if (rc)
		return rc;
	std::lock_guard<std::mutex> g(c->lock);

	hipSetDevice(c->device);
	/* the previous upload read t->blob asynchronously */
	if (t->uploaded && hipEventSynchronize(t->uploaded) != hipSuccess)
		return -EIO;
	if (!t->uploaded && hipEventCreateWithFlags(&t->uploaded, hipEventDisableTiming) != hipSuccess)
		return -EIO;
	if (hdr.blob_bytes > t->cap) {
		void *nb = nullptr;

		/* launches still reading the old allocation end first */
		if (hipStreamSynchronize(ctx_stream_locked(c)) != hipSuccess ||
		    hipMalloc(&nb, hdr.blob_bytes) != hipSuccess)
			return -ENOMEM;
		hipFree(t->dblob);
		t->dblob = nb;
		t->cap = hdr.blob_bytes;
	}
	t->blob.swap(blob);
	t->hdr = hdr;
	t->cycle = odpg_rules_has_cycle(t->blob, t->hdr);
	t->depth = table_walk_depth(t);
	t->qsig = table_qsig(t);
	hipStream_t cs = ctx_stream_locked(c);

	if (hipMemcpyAsync(t->dblob, t->blob.data(), t->hdr.blob_bytes, hipMemcpyHostToDevice,
			   cs) != hipSuccess ||
	    hipEventRecord(t->uploaded, cs) != hipSuccess)
		return -EIO;
	return 0;
}

void odpg_table_destroy(odpg_table_t *t)
{
	if (!t)
		return;
	hipSetDevice(t->device);
	if (t->uploaded) {
		hipEventSynchronize(t->uploaded);
		hipEventDestroy(t->uploaded);
	}
	hipFree(t->dblob);
	delete t;
}

uint32_t odpg_table_num_cos(const odpg_table_t *t)
{
	return t ? t->hdr.num_cos : 0;
}

int odpg_table_has_cycle(const odpg_table_t *t)
{
	return t ? t->cycle : 0;
}

/* ---- sharded counters ---------------------------------------------------- */
#define CNT_ROWS_PER_CU 8u
#define CNT_MAX_BYTES   (512ull << 20)
#define CNT_MAX_LDS     (48u << 10)   /* LDS histograms of one workgroup */

extern "C" int odpg_launch_counters_fold(uint64_t *rows, uint32_t nrows, uint32_t words,
					 uint64_t *sum, hipStream_t s);

/* queue columns of a table: CoS c has nq[c] = max(num_queue, 1) queues, the
 * first in column qcol[c]; qcol[num_cos] = the columns in all (the layout of
 * the sharded counters' delivery block and of the delivery lists' buckets) */
static void table_queue_cols(const odpg_table_t *t, std::vector<uint32_t> &qcol,
			     std::vector<uint8_t> &nq)
{
	const dcos_t *hc = (const dcos_t *)(t->blob.data() + t->hdr.cos_off);
	const uint32_t n = t->hdr.num_cos;
	uint32_t col = 0;

	qcol.resize(n + 1u);
	nq.resize(n);
	for (uint32_t i = 0; i < n; i++) {
		qcol[i] = col;
		nq[i] = (uint8_t)(hc[i].num_queue ? hc[i].num_queue : 1u);
		col += nq[i];
	}
	qcol[n] = col;
}

static void counters_free(odpg_counters_t *k)
{
	odpg_ctx_t *c = k->ctx;

	hipFree(k->drows);
	hipFree(k->dqcol);
	hipFree(k->dsum);
	if (k->hsum)
		hipHostFree(k->hsum);
	if (k->done)
		hipEventDestroy(k->done);
	delete k;
	odpg_ctx_unref(c);
}

int odpg_counters_create(odpg_ctx_t *c, const odpg_table_t *t, odpg_counters_t **out)
{
	if (!c || !t || !out)
		return -EINVAL;
	if (t->device != c->device)
		return -EXDEV;
	const dtable_hdr_t &h = t->hdr;
	const dcos_t *hc = (const dcos_t *)(t->blob.data() + h.cos_off);
	odpg_counters_t *k = new odpg_counters_t();

	k->ctx = c;
	odpg_ctx_ref(c);
	k->qsig = t->qsig;
	k->ncos = h.num_cos;
	table_queue_cols(t, k->qcol, k->nq);
	for (uint32_t i = 0; i < h.num_cos; i++)
		k->any_cos |= hc[i].stats ? 1u : 0u;
	k->ncols = k->qcol[h.num_cos];
	k->words = 4u + k->ncos + k->ncols;
	if (((size_t)k->ncos + k->ncols) * 4u > CNT_MAX_LDS) {
		counters_free(k);
		return -E2BIG;
	}
	int cus = 0;

	hipSetDevice(c->device);
	if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device) != hipSuccess ||
	    cus <= 0)
		cus = 256;
	k->rows = (uint32_t)cus * CNT_ROWS_PER_CU;
	while (k->rows > (uint32_t)cus && (size_t)k->rows * k->words * 8u > CNT_MAX_BYTES)
		k->rows >>= 1;
	if ((size_t)k->rows * k->words * 8u > CNT_MAX_BYTES) {
		counters_free(k);
		return -E2BIG;
	}
	/* a set of rows per launch lane, so that launches on both lanes never
	 * share a row; where two sets do not fit the object keeps one and its
	 * launches stay on the context stream */
	k->sets = c->lane1 && 2u * ((size_t)k->rows * k->words * 8u) <= CNT_MAX_BYTES ? 2u : 1u;
	const size_t rb = (size_t)k->sets * k->rows * k->words * 8u;

	if (hipMalloc(&k->drows, rb) != hipSuccess ||
	    hipMalloc(&k->dqcol, (size_t)(k->ncos + 1u) * 4u) != hipSuccess ||
	    hipMalloc(&k->dsum, (size_t)k->words * 8u) != hipSuccess ||
	    hipHostMalloc(&k->hsum, (size_t)k->words * 8u, hipHostMallocDefault) != hipSuccess ||
	    hipEventCreateWithFlags(&k->done, hipEventDisableTiming) != hipSuccess) {
		counters_free(k);
		return -ENOMEM;
	}
	{
		std::lock_guard<std::mutex> g(c->lock);
		hipStream_t cs = ctx_stream_locked(c);

		if (hipMemsetAsync(k->drows, 0, rb, cs) != hipSuccess ||
		    hipMemsetAsync(k->dsum, 0, (size_t)k->words * 8u, cs) != hipSuccess ||
		    hipMemcpyAsync(k->dqcol, k->qcol.data(), (size_t)(k->ncos + 1u) * 4u,
				   hipMemcpyHostToDevice, cs) != hipSuccess ||
		    hipEventRecord(k->done, cs) != hipSuccess) {
			counters_free(k);
			return -EIO;
		}
	}
	if (hipEventSynchronize(k->done) != hipSuccess) {
		counters_free(k);
		return -EIO;
	}
	*out = k;
	return 0;
}

int odpg_counters_match(const odpg_counters_t *k, const odpg_table_t *t)
{
	return k && t && k->qsig == t->qsig && k->ncos == t->hdr.num_cos;
}

void odpg_counters_destroy(odpg_counters_t *k)
{
	if (!k)
		return;
	hipSetDevice(k->ctx->device);
	hipStreamSynchronize(ctx_stream(k->ctx));   /* launches still adding into the rows */
	counters_free(k);
}

/* sum and clear row sets [set0, set0 + nsets) into `words` */
static int counters_fold_sets(odpg_counters_t *k, uint32_t set0, uint32_t nsets, uint64_t *words)
{
	odpg_ctx_t *c = k->ctx;
	std::lock_guard<std::mutex> fl(k->lock);

	hipSetDevice(c->device);
	{
		/* enqueue behind every launch already on the context stream */
		std::lock_guard<std::mutex> g(c->lock);
		hipStream_t cs = ctx_stream_locked(c);

		if (odpg_launch_counters_fold(k->drows + (size_t)set0 * k->rows * k->words,
					      nsets * k->rows, k->words, k->dsum, cs) ||
		    hipMemcpyAsync(k->hsum, k->dsum, (size_t)k->words * 8u, hipMemcpyDeviceToHost,
				   cs) != hipSuccess ||
		    hipMemsetAsync(k->dsum, 0, (size_t)k->words * 8u, cs) != hipSuccess ||
		    hipEventRecord(k->done, cs) != hipSuccess)
			return -EIO;
	}
	HIPCHK(hipEventSynchronize(k->done));
	for (uint32_t w = 0; w < 4u + k->ncos; w++)
		words[w] += k->hsum[w];
	const uint64_t *dl = k->hsum + 4u + k->ncos;
	uint64_t *uq = words + 4u + k->ncos;

	for (uint32_t i = 0; i < k->ncos; i++)
		for (uint32_t q = 0; q < k->nq[i]; q++)
			uq[(size_t)i * ODPG_COS_QUEUE_MAX + q] += dl[k->qcol[i] + q];
	return 0;
}

int odpg_counters_fold(odpg_counters_t *k, uint64_t *words)
{
	if (!k || !words)
		return -EINVAL;
	return counters_fold_sets(k, 0, k->sets, words);
}

/* odpg_internal.h: the rows launches on `lane` added into, for the tests */
int odpg_counters_fold_lane(odpg_counters_t *k, int lane, uint64_t *words)
{
	if (!k || !words || lane < 0 || (uint32_t)lane >= k->sets)
		return -EINVAL;
	return counters_fold_sets(k, (uint32_t)lane, 1, words);
}

/* ---- delivery lists (odpg_deliver.h; kernels in deliver.hip) ------------- */
struct odpg_deliver_s {
	odpg_ctx_t *ctx;
	uint32_t max_pkts;
	std::vector<uint32_t> qcol;    /* host: qbase, ncos + 1 */
	std::vector<uint8_t> nq;
	odpg_deliver_args a;           /* layout + device workspace */
};

static void deliver_free(odpg_deliver_t *d)
{
	odpg_ctx_t *c = d->ctx;

	hipFree((void *)d->a.qbase);
	hipFree(d->a.hist);
	hipFree(d->a.dtotal);
	hipFree(d->a.bcount);
	hipFree(d->a.pairs);
	delete d;
	odpg_ctx_unref(c);
}

int odpg_deliver_create(odpg_ctx_t *c, const odpg_table_t *t, uint32_t max_pkts,
			odpg_deliver_t **out)
{
	/* packet positions and tile starts are 32-bit sums below 2^32 */
	if (!c || !t || !out || max_pkts > (1u << 31))
		return -EINVAL;
	if (t->device != c->device)
		return -EXDEV;
	odpg_deliver_t *d = new odpg_deliver_t();
	odpg_deliver_args &a = d->a;

	d->ctx = c;
	odpg_ctx_ref(c);
	d->max_pkts = max_pkts;
	table_queue_cols(t, d->qcol, d->nq);
	a.num_cos = t->hdr.num_cos;
	a.nbuckets = d->qcol[a.num_cos] + 2u;
	a.key_bits = dlv_key_bits(a.nbuckets);
	const bool two = a.key_bits > DLV_DIGIT_BITS;
	const size_t tiles = ((size_t)max_pkts + DLV_TILE - 1u) / DLV_TILE;
	const size_t hist_words = std::max<size_t>(tiles, 1u) << dlv_bits0(a.key_bits);
	const size_t qb = (size_t)(a.num_cos + 1u) * 4u;
	hipEvent_t ready = nullptr;
	int rc = -ENOMEM;

	hipSetDevice(c->device);
	if (hipMalloc((void **)&a.qbase, qb) == hipSuccess &&
	    hipMalloc(&a.hist, hist_words * 4u) == hipSuccess &&
	    hipMalloc(&a.dtotal, DLV_RADIX * 4u) == hipSuccess &&
	    (!two || (hipMalloc(&a.bcount, (size_t)a.nbuckets * 4u) == hipSuccess &&
		      hipMalloc(&a.pairs, std::max<size_t>(max_pkts, 1u) * 8u) == hipSuccess)) &&
	    hipEventCreateWithFlags(&ready, hipEventDisableTiming) == hipSuccess) {
		std::lock_guard<std::mutex> g(c->lock);
		hipStream_t cs = ctx_stream_locked(c);

		rc = -EIO;
		if (hipMemcpyAsync((void *)a.qbase, d->qcol.data(), qb, hipMemcpyHostToDevice,
				   cs) == hipSuccess &&
		    odpg_launch_deliver_clear(a.dtotal, DLV_RADIX, cs) == 0 &&
		    (!two || odpg_launch_deliver_clear(a.bcount, a.nbuckets, cs) == 0) &&
		    hipEventRecord(ready, cs) == hipSuccess)
			rc = 0;
	}
	/* the upload reads d->qcol: done before the plan is handed out */
	if (rc == 0 && hipEventSynchronize(ready) != hipSuccess)
		rc = -EIO;
	if (ready)
		hipEventDestroy(ready);
	if (rc) {
		deliver_free(d);
		return rc;
	}
	*out = d;
	return 0;
}

void odpg_deliver_destroy(odpg_deliver_t *d)
{
	if (!d)
		return;
	hipSetDevice(d->ctx->device);
	hipStreamSynchronize(ctx_stream(d->ctx));   /* launches still using the workspace */
	deliver_free(d);
}

uint32_t odpg_deliver_num_buckets(const odpg_deliver_t *d)
{
	return d ? d->a.nbuckets : 0u;
}

int odpg_deliver_queue_base(const odpg_deliver_t *d, uint32_t cos)
{
	if (!d || cos >= d->a.num_cos)
		return -EINVAL;
	return (int)d->qcol[cos];
}

int odpg_deliver_match(const odpg_deliver_t *d, const odpg_table_t *t)
{
	if (!d || !t || d->a.num_cos != t->hdr.num_cos)
		return 0;
	const dcos_t *hc = (const dcos_t *)(t->blob.data() + t->hdr.cos_off);

	for (uint32_t i = 0; i < d->a.num_cos; i++)
		if (d->nq[i] != (hc[i].num_queue ? hc[i].num_queue : 1u))
			return 0;
	return 1;
}

int odpg_deliver(odpg_deliver_t *d, const odpg_out_t *out, uint32_t num, uint32_t *order,
		 uint32_t *offsets)
{
	if (!d || !out || !order || !offsets || num > d->max_pkts)
		return -EINVAL;
	odpg_ctx_t *c = d->ctx;
	odpg_deliver_args a = d->a;

	a.out = out;
	a.num = num;
	a.order = order;
	a.offsets = offsets;
	hipSetDevice(c->device);
	std::lock_guard<std::mutex> g(c->lock);

	return odpg_launch_deliver(&a, ctx_stream_locked(c));
}

/* ---- dense queue batches (odpg_gather.h; kernels in gather.hip) ----------- */
struct odpg_gather_s {
	odpg_ctx_t *ctx;
	uint32_t max_pkts;
	uint64_t *tsum;                /* device: a word per tile */
	odpg_desc_t *pos;              /* device: max_pkts source descriptors */
};

static void gather_free(odpg_gather_t *g)
{
	odpg_ctx_t *c = g->ctx;

	hipFree(g->tsum);
	hipFree(g->pos);
	delete g;
	odpg_ctx_unref(c);
}

int odpg_gather_create(odpg_ctx_t *c, uint32_t max_pkts, odpg_gather_t **out)
{
	/* positions are 32-bit sums below 2^32, as in a delivery plan */
	if (!c || !out || max_pkts > (1u << 31))
		return -EINVAL;
	odpg_gather_t *g = new odpg_gather_t();
	const size_t tiles = ((size_t)max_pkts + GTH_TILE - 1u) / GTH_TILE;

	g->ctx = c;
	odpg_ctx_ref(c);
	g->max_pkts = max_pkts;
	hipSetDevice(c->device);
	if (hipMalloc(&g->tsum, std::max<size_t>(tiles, 1u) * 8u) != hipSuccess ||
	    hipMalloc(&g->pos, std::max<size_t>(max_pkts, 1u) * sizeof(odpg_desc_t)) != hipSuccess) {
		gather_free(g);
		return -ENOMEM;
	}
	*out = g;
	return 0;
}

void odpg_gather_destroy(odpg_gather_t *g)
{
	if (!g)
		return;
	hipSetDevice(g->ctx->device);
	hipStreamSynchronize(ctx_stream(g->ctx));   /* launches still using the workspace */
	gather_free(g);
}

int odpg_gather(odpg_gather_t *g, const odpg_gather_src_t *src, const uint32_t *order,
		const uint32_t *offsets, uint32_t b_first, uint32_t b_last,
		const odpg_gather_dst_t *dst)
{
	if (!g || !src || !order || !offsets || !dst || !dst->frames || !dst->total ||
	    (!src->frames && src->num) || (((uintptr_t)src->frames | (uintptr_t)dst->frames) & 15u) ||
	    src->num > g->max_pkts || b_first > b_last || dst->capacity > (1ull << 32) ||
	    (!src->desc && (!src->stride || (src->stride & 15u))) || (src->desc && !dst->desc) ||
	    !src->words != !dst->words)
		return -EINVAL;
	odpg_ctx_t *c = g->ctx;
	odpg_gather_args a = {*src, *dst, order, offsets, b_first, b_last, g->tsum, g->pos};

	hipSetDevice(c->device);
	std::lock_guard<std::mutex> lk(c->lock);

	return odpg_launch_gather(&a, ctx_stream_locked(c));
}

/* ---- segmentation offload (odpg_lso.h; kernels in lso.hip) ----------------- */
struct odpg_lso_s {
	odpg_ctx_t *ctx;
	uint32_t max_pkts, num_profiles;
	odpg_lso_profile_t *profiles;  /* device */
	odpg_lso_pk *pk;               /* device: max_pkts records */
	uint64_t *tunits;              /* device: a word per tile, each */
	uint32_t *tsegs, *tbad;
};

/* odp_lso_profile_create (odp_packet_io.c:2836-2885) */
int odpg_lso_profile_check(const odpg_lso_profile_t *p)
{
	if (!p || (p->proto != ODPG_LSO_PROTO_IPV4 && p->proto != ODPG_LSO_PROTO_CUSTOM))
		return -EINVAL;
	if (p->proto != ODPG_LSO_PROTO_CUSTOM)
		return 0;
	if (p->num_custom > ODPG_LSO_MAX_CUSTOM)
		return -EINVAL;
	for (uint32_t i = 0; i < p->num_custom; i++) {
		const odpg_lso_field_t &f = p->field[i];

		if (f.offset > ODPG_LSO_MAX_PAYLOAD_OFFSET ||
		    (f.mod_op != ODPG_LSO_ADD_SEGMENT_NUM && f.mod_op != ODPG_LSO_WRITE_BITS) ||
		    (f.mod_op == ODPG_LSO_WRITE_BITS && f.size != 1u) ||
		    (f.size != 1u && f.size != 2u && f.size != 4u && f.size != 8u))
			return -EINVAL;
	}
	return 0;
}

static void lso_free(odpg_lso_t *l)
{
	odpg_ctx_t *c = l->ctx;

	hipFree(l->profiles);
	hipFree(l->pk);
	hipFree(l->tunits);
	hipFree(l->tsegs);
	hipFree(l->tbad);
	delete l;
	odpg_ctx_unref(c);
}

int odpg_lso_create(odpg_ctx_t *c, const odpg_lso_profile_t *profiles, uint32_t num_profiles,
		    uint32_t max_pkts, odpg_lso_t **out)
{
	/* 64 segments a packet: positions stay below 2^32 */
	if (!c || !profiles || !out || !num_profiles || num_profiles > ODPG_LSO_MAX_PROFILES ||
	    max_pkts > (1u << 25))
		return -EINVAL;
	for (uint32_t i = 0; i < num_profiles; i++)
		if (odpg_lso_profile_check(&profiles[i]))
			return -EINVAL;
	odpg_lso_t *l = new odpg_lso_t();
	const size_t tiles = std::max<size_t>(((size_t)max_pkts + LSO_TILE - 1u) / LSO_TILE, 1u);
	const size_t pb = num_profiles * sizeof(odpg_lso_profile_t);
	int rc = -ENOMEM;

	l->ctx = c;
	odpg_ctx_ref(c);
	l->max_pkts = max_pkts;
	l->num_profiles = num_profiles;
	hipSetDevice(c->device);
	if (hipMalloc(&l->profiles, pb) == hipSuccess &&
	    hipMalloc(&l->pk, std::max<size_t>(max_pkts, 1u) * sizeof(odpg_lso_pk)) == hipSuccess &&
	    hipMalloc(&l->tunits, tiles * 8u) == hipSuccess &&
	    hipMalloc(&l->tsegs, tiles * 4u) == hipSuccess &&
	    hipMalloc(&l->tbad, tiles * 4u) == hipSuccess)
		/* synchronous: `profiles` is the caller's again on return */
		rc = hipMemcpy(l->profiles, profiles, pb, hipMemcpyHostToDevice) == hipSuccess ? 0 : -EIO;
	if (rc) {
		lso_free(l);
		return rc;
	}
	*out = l;
	return 0;
}

void odpg_lso_destroy(odpg_lso_t *l)
{
	if (!l)
		return;
	hipSetDevice(l->ctx->device);
	hipStreamSynchronize(ctx_stream(l->ctx));   /* launches still using the workspace */
	lso_free(l);
}

int odpg_lso(odpg_lso_t *l, const odpg_lso_src_t *src, const odpg_lso_dst_t *dst)
{
	if (!l || !src || !dst || !dst->frames || !dst->seg_first || !dst->status || !dst->total ||
	    (!dst->desc && dst->max_segs) || (!src->frames && src->num) ||
	    (((uintptr_t)src->frames | (uintptr_t)dst->frames) & 15u) || src->num > l->max_pkts ||
	    (!src->desc && (!src->stride || (src->stride & 15u))) || dst->capacity > (1ull << 32))
		return -EINVAL;
	odpg_ctx_t *c = l->ctx;
	odpg_lso_args a = {*src, *dst, l->profiles, l->num_profiles, l->pk, l->tunits, l->tsegs,
			   l->tbad};

	hipSetDevice(c->device);
	std::lock_guard<std::mutex> lk(c->lock);

	return odpg_launch_lso(&a, ctx_stream_locked(c));
}

/* ---- IPv4 reassembly (odpg_reass.h; kernels in reass.hip) ------------------- */
struct odpg_reass_s {
	odpg_ctx_t *ctx;
	uint32_t max_pkts;
	odpg_reass_pk *pk;             /* device: max_pkts records, each */
	odpg_reass_grp *grp;
	uint32_t *lead, *obase;
	uint32_t *flow;                /* device: pow2 >= 2 max_pkts slots, each */
	unsigned long long *pos;
	uint64_t *tunits;              /* device: a word per tile, each */
	uint32_t *touts, *theld, *tbad;
};

/* the smallest power of two >= 2 n, at least 64 */
static uint32_t reass_slots(uint32_t n)
{
	uint32_t s = 64;

	while (s < 2u * n)
		s <<= 1;
	return s;
}

static void reass_free(odpg_reass_t *r)
{
	odpg_ctx_t *c = r->ctx;

	hipFree(r->pk);
	hipFree(r->grp);
	hipFree(r->lead);
	hipFree(r->obase);
	hipFree(r->flow);
	hipFree(r->pos);
	hipFree(r->tunits);
	hipFree(r->touts);
	hipFree(r->theld);
	hipFree(r->tbad);
	delete r;
	odpg_ctx_unref(c);
}

int odpg_reass_create(odpg_ctx_t *c, uint32_t max_pkts, odpg_reass_t **out)
{
	/* a leader's index shares a 64-bit key with a byte position; 2 * 2^24 slots */
	if (!c || !out || max_pkts > (1u << 24))
		return -EINVAL;
	odpg_reass_t *r = new odpg_reass_t();
	const size_t n = std::max<size_t>(max_pkts, 1u), slots = reass_slots(max_pkts);
	const size_t tiles = (n + REASS_TILE - 1u) / REASS_TILE;

	r->ctx = c;
	odpg_ctx_ref(c);
	r->max_pkts = max_pkts;
	hipSetDevice(c->device);
	if (hipMalloc(&r->pk, n * sizeof(odpg_reass_pk)) != hipSuccess ||
	    hipMalloc(&r->grp, n * sizeof(odpg_reass_grp)) != hipSuccess ||
	    hipMalloc(&r->lead, n * 4u) != hipSuccess || hipMalloc(&r->obase, n * 4u) != hipSuccess ||
	    hipMalloc(&r->flow, slots * 4u) != hipSuccess ||
	    hipMalloc(&r->pos, slots * 8u) != hipSuccess ||
	    hipMalloc(&r->tunits, tiles * 8u) != hipSuccess ||
	    hipMalloc(&r->touts, tiles * 4u) != hipSuccess ||
	    hipMalloc(&r->theld, tiles * 4u) != hipSuccess ||
	    hipMalloc(&r->tbad, tiles * 4u) != hipSuccess) {
		reass_free(r);
		return -ENOMEM;
	}
	*out = r;
	return 0;
}

void odpg_reass_destroy(odpg_reass_t *r)
{
	if (!r)
		return;
	hipSetDevice(r->ctx->device);
	hipStreamSynchronize(ctx_stream(r->ctx));   /* launches still using the workspace */
	reass_free(r);
}

int odpg_reass(odpg_reass_t *r, const odpg_reass_src_t *src, const odpg_reass_dst_t *dst)
{
	if (!r || !src || !dst || !dst->frames || !dst->status || !dst->held || !dst->held_offsets ||
	    !dst->total || ((!dst->desc || !dst->origin) && dst->max_out) ||
	    (!src->frames && src->num) ||
	    (((uintptr_t)src->frames | (uintptr_t)dst->frames) & 15u) || src->num > r->max_pkts ||
	    (!src->desc && (!src->stride || (src->stride & 15u))) ||
	    (src->l3_offset && (((uintptr_t)src->l3_offset & 1u) || !src->l3_stride ||
				(src->l3_stride & 1u))) ||
	    dst->capacity > (1ull << 32))
		return -EINVAL;
	odpg_ctx_t *c = r->ctx;
	/* tables sized for this batch: clearing them costs what the batch is worth */
	odpg_reass_args a = {*src, *dst, r->pk, r->grp, r->lead, r->obase, r->flow, r->pos,
			     reass_slots(src->num), 0, r->tunits, r->touts, r->theld, r->tbad};

	hipSetDevice(c->device);
	std::lock_guard<std::mutex> lk(c->lock);

	return odpg_launch_reass(&a, ctx_stream_locked(c));
}

/* ---- L2 switch (odpg_switch.h; kernels in switch.hip) ------------------------ */
struct odpg_switch_s {
	odpg_ctx_t *ctx;
	uint32_t max_pkts;
	odpg_switch_args a;            /* ports, table and device workspace */
};

static void switch_free(odpg_switch_t *w)
{
	odpg_ctx_t *c = w->ctx;

	hipFree(w->a.table);
	hipFree(w->a.rec);
	hipFree(w->a.skey);
	hipFree(w->a.mask);
	hipFree(w->a.order);
	hipFree(w->a.offsets);
	hipFree(w->a.tcnt);
	hipFree(w->a.hist);
	hipFree(w->a.dtotal);
	hipFree(w->a.bcount);
	hipFree(w->a.pairs);
	delete w;
	odpg_ctx_unref(c);
}

int odpg_switch_create(odpg_ctx_t *c, uint32_t num_ports, uint32_t max_pkts, odpg_switch_t **out)
{
	/* a writer run's binary search and the tile counts rely on num <= 2^24 */
	if (!c || !out || num_ports < 2u || num_ports > ODPG_SWITCH_MAX_PORTS ||
	    max_pkts > (1u << 24))
		return -EINVAL;
	odpg_switch_t *w = new odpg_switch_t();
	odpg_switch_args &a = w->a;
	const size_t n = std::max<size_t>(max_pkts, 1u);
	const size_t tiles = (n + SW_TILE - 1u) / SW_TILE;
	const size_t hist_words = ((n + DLV_TILE - 1u) / DLV_TILE) << dlv_bits0(SW_KEY_BITS);
	int rc = -ENOMEM;

	w->ctx = c;
	odpg_ctx_ref(c);
	w->max_pkts = max_pkts;
	a.num_ports = num_ports;
	hipSetDevice(c->device);
	if (hipMalloc(&a.table, (size_t)SW_SLOTS * 8u) == hipSuccess &&
	    hipMalloc(&a.rec, n * sizeof(odpg_switch_rec)) == hipSuccess &&
	    hipMalloc(&a.skey, n * 4u) == hipSuccess && hipMalloc(&a.mask, n * 4u) == hipSuccess &&
	    hipMalloc(&a.order, n * 4u) == hipSuccess &&
	    hipMalloc(&a.offsets, (size_t)(SW_BUCKETS + 1u) * 4u) == hipSuccess &&
	    hipMalloc(&a.tcnt, tiles * SW_COLS * 4u) == hipSuccess &&
	    hipMalloc(&a.hist, hist_words * 4u) == hipSuccess &&
	    hipMalloc(&a.dtotal, DLV_RADIX * 4u) == hipSuccess &&
	    hipMalloc(&a.bcount, (size_t)SW_BUCKETS * 4u) == hipSuccess &&
	    hipMalloc(&a.pairs, n * 8u) == hipSuccess) {
		std::lock_guard<std::mutex> g(c->lock);
		hipStream_t cs = ctx_stream_locked(c);

		/* on the context stream, like every later call and table copy */
		rc = odpg_launch_switch_clear((uint32_t *)a.table, SW_SLOTS * 2u, cs) == 0 &&
		     odpg_launch_switch_clear(a.dtotal, DLV_RADIX, cs) == 0 &&
		     odpg_launch_switch_clear(a.bcount, SW_BUCKETS, cs) == 0 ? 0 : -EIO;
	}
	if (rc) {
		switch_free(w);
		return rc;
	}
	*out = w;
	return 0;
}

void odpg_switch_destroy(odpg_switch_t *w)
{
	if (!w)
		return;
	hipSetDevice(w->ctx->device);
	hipStreamSynchronize(ctx_stream(w->ctx));   /* launches still using the workspace */
	switch_free(w);
}

uint64_t *odpg_switch_table(odpg_switch_t *w)
{
	return w ? w->a.table : nullptr;
}

int odpg_switch(odpg_switch_t *w, const odpg_switch_src_t *src, uint8_t cur_tick,
		const odpg_switch_dst_t *dst)
{
	if (!w || !src || !dst || !dst->out || !dst->lists || !dst->port_offsets || !dst->total ||
	    (!src->frames && src->num) || ((uintptr_t)src->frames & 15u) ||
	    (!src->desc && (!src->stride || (src->stride & 15u))) || src->num > w->max_pkts ||
	    dst->list_stride < src->num)
		return -EINVAL;
	odpg_ctx_t *c = w->ctx;
	odpg_switch_args a = w->a;

	a.src = *src;
	a.dst = *dst;
	a.cur_tick = cur_tick;
	hipSetDevice(c->device);
	std::lock_guard<std::mutex> lk(c->lock);

	return odpg_launch_switch(&a, ctx_stream_locked(c));
}

/* ---- ESP tunnel AES-GCM (odpg_esp.h; kernels in esp.hip) ---------------------- */
struct odpg_esp_s {
	odpg_ctx_t *ctx;
	uint32_t max_pkts;
	odpg_esp_sa_dev *sas;          /* device */
	uint32_t *te0;                 /* device */
	odpg_esp_args a;               /* direction, SAs and device workspace */
};

/* S-box by the walk over the powers of the generator 3 and their inverses,
 * then te0[x] = {02, 01, 01, 03} . S[x] (esp.h) */
static const uint32_t *esp_te0()
{
	static uint32_t te0[256];
	static std::once_flag once;

	std::call_once(once, [] {
		uint8_t sbox[256], p = 1, q = 1;

		do {
			p = (uint8_t)(p ^ (p << 1) ^ ((p & 0x80u) ? 0x1Bu : 0u));
			q ^= (uint8_t)(q << 1);
			q ^= (uint8_t)(q << 2);
			q ^= (uint8_t)(q << 4);
			q ^= (q & 0x80u) ? 0x09u : 0u;
			const uint8_t x = (uint8_t)(q ^ (q << 1 | q >> 7) ^ (q << 2 | q >> 6) ^
						    (q << 3 | q >> 5) ^ (q << 4 | q >> 4));
			sbox[p] = x ^ 0x63u;
		} while (p != 1);
		sbox[0] = 0x63u;
		for (uint32_t i = 0; i < 256u; i++) {
			const uint32_t s = sbox[i], s2 = ((s << 1) ^ ((s & 0x80u) ? 0x11Bu : 0u)) & 0xFFu;

			te0[i] = s2 << 24 | s << 16 | s << 8 | (s2 ^ s);
		}
	});
	return te0;
}

int odpg_esp_key_schedule(const uint8_t *key, uint32_t key_len, uint32_t rk[60], uint8_t h[16])
{
	if (!key || !rk || !h || (key_len != 16u && key_len != 24u && key_len != 32u))
		return -EINVAL;
	const uint32_t *te0 = esp_te0();
	const uint32_t nk = key_len / 4u, nr = nk + 6u, words = 4u * (nr + 1u);
	uint32_t rcon = 1, z[4] = {0u, 0u, 0u, 0u};
	auto sub = [te0](uint32_t w) {
		return ((te0[w >> 24] >> 8) & 0xFFu) << 24 | ((te0[(w >> 16) & 0xFFu] >> 8) & 0xFFu) << 16 |
		       ((te0[(w >> 8) & 0xFFu] >> 8) & 0xFFu) << 8 | ((te0[w & 0xFFu] >> 8) & 0xFFu);
	};

	memset(rk, 0, 60u * sizeof(uint32_t));
	for (uint32_t i = 0; i < nk; i++)
		rk[i] = (uint32_t)key[4 * i] << 24 | (uint32_t)key[4 * i + 1] << 16 |
			(uint32_t)key[4 * i + 2] << 8 | key[4 * i + 3];
	for (uint32_t i = nk; i < words; i++) {
		uint32_t t = rk[i - 1];

		if (i % nk == 0) {
			t = sub(t << 8 | t >> 24) ^ rcon << 24;
			rcon = ((rcon << 1) ^ ((rcon & 0x80u) ? 0x11Bu : 0u)) & 0xFFu;
		} else if (nk > 6u && i % nk == 4u) {
			t = sub(t);
		}
		rk[i] = rk[i - nk] ^ t;
	}
	esp_aes_encrypt(rk, nr, te0, z);
	for (uint32_t i = 0; i < 16u; i++)
		h[i] = (uint8_t)(z[i >> 2] >> (24u - 8u * (i & 3u)));
	return 0;
}

static void esp_free(odpg_esp_t *e)
{
	odpg_ctx_t *c = e->ctx;
	odpg_esp_args &a = e->a;

	hipFree(e->sas);
	hipFree(e->te0);
	hipFree(a.next_seq);
	hipFree(a.rec);
	hipFree(a.ounit);
	hipFree(a.seq64);
	hipFree(a.tunits);
	hipFree(a.tok);
	hipFree(a.tbad);
	hipFree(a.skey);
	hipFree(a.order);
	hipFree(a.offsets);
	hipFree(a.hist);
	hipFree(a.dtotal);
	hipFree(a.bcount);
	hipFree(a.pairs);
	delete e;
	odpg_ctx_unref(c);
}

int odpg_esp_create(odpg_ctx_t *c, uint32_t dir, uint32_t max_sas, uint32_t max_pkts,
		    odpg_esp_t **out)
{
	if (!c || !out || (dir != ODPG_ESP_OUT && dir != ODPG_ESP_IN) || !max_sas ||
	    max_sas > ODPG_ESP_MAX_SAS || max_pkts > (1u << 24))
		return -EINVAL;
	odpg_esp_t *e = new odpg_esp_t();
	odpg_esp_args &a = e->a;
	const size_t n = std::max<size_t>(max_pkts, 1u);
	const size_t tiles = (n + ESP_PREP_WG - 1u) / ESP_PREP_WG;
	const bool is_out = dir == ODPG_ESP_OUT;
	const size_t sa_words = (size_t)max_sas * sizeof(odpg_esp_sa_dev) / 4u;
	int rc = -ENOMEM;

	e->ctx = c;
	odpg_ctx_ref(c);
	e->max_pkts = max_pkts;
	a.dir = dir;
	a.max_sas = max_sas;
	a.key_bits = dlv_key_bits(max_sas + 1u);
	const size_t hist_words = ((n + DLV_TILE - 1u) / DLV_TILE) << dlv_bits0(a.key_bits);
	const bool two = a.key_bits > DLV_DIGIT_BITS;

	hipSetDevice(c->device);
	if (hipMalloc(&e->sas, sa_words * 4u) == hipSuccess &&
	    hipMalloc(&e->te0, 1024u) == hipSuccess &&
	    hipMalloc(&a.rec, n * sizeof(odpg_esp_rec)) == hipSuccess &&
	    hipMalloc(&a.ounit, n * 4u) == hipSuccess &&
	    hipMalloc(&a.tunits, tiles * 8u) == hipSuccess &&
	    hipMalloc(&a.tok, tiles * 4u) == hipSuccess && hipMalloc(&a.tbad, tiles * 4u) == hipSuccess &&
	    (!is_out ||
	     (hipMalloc(&a.next_seq, (size_t)max_sas * 8u) == hipSuccess &&
	      hipMalloc(&a.seq64, n * 8u) == hipSuccess && hipMalloc(&a.skey, n * 4u) == hipSuccess &&
	      hipMalloc(&a.order, n * 4u) == hipSuccess &&
	      hipMalloc(&a.offsets, (size_t)(max_sas + 2u) * 4u) == hipSuccess &&
	      hipMalloc(&a.hist, hist_words * 4u) == hipSuccess &&
	      hipMalloc(&a.dtotal, DLV_RADIX * 4u) == hipSuccess &&
	      (!two || (hipMalloc(&a.bcount, (size_t)(max_sas + 1u) * 4u) == hipSuccess &&
			hipMalloc(&a.pairs, n * 8u) == hipSuccess))))) {
		std::lock_guard<std::mutex> g(c->lock);
		hipStream_t cs = ctx_stream_locked(c);

		/* on the context stream, like every later call and SA upload */
		rc = hipMemcpyAsync(e->te0, esp_te0(), 1024u, hipMemcpyHostToDevice, cs) == hipSuccess &&
		     odpg_launch_esp_clear((uint32_t *)e->sas, (uint32_t)sa_words, cs) == 0 &&
		     (!is_out ||
		      (odpg_launch_esp_clear((uint32_t *)a.next_seq, max_sas * 2u, cs) == 0 &&
		       odpg_launch_esp_clear(a.dtotal, DLV_RADIX, cs) == 0 &&
		       (!two || odpg_launch_esp_clear(a.bcount, max_sas + 1u, cs) == 0))) ? 0 : -EIO;
	}
	if (rc) {
		esp_free(e);
		return rc;
	}
	a.sas = e->sas;
	a.te0 = e->te0;
	*out = e;
	return 0;
}

void odpg_esp_destroy(odpg_esp_t *e)
{
	if (!e)
		return;
	hipSetDevice(e->ctx->device);
	hipStreamSynchronize(ctx_stream(e->ctx));   /* launches still using the workspace */
	esp_free(e);
}

uint64_t *odpg_esp_next_seq(odpg_esp_t *e)
{
	return e ? e->a.next_seq : nullptr;
}

int odpg_esp_sa_set(odpg_esp_t *e, uint32_t index, const odpg_esp_sa_t *sa)
{
	if (!e || index >= e->a.max_sas)
		return -EINVAL;
	odpg_esp_sa_dev d;
	const uint64_t one = 1;

	memset(&d, 0, sizeof(d));
	if (sa) {
		uint8_t h[16];

		if (odpg_esp_key_schedule(sa->key, sa->key_len, d.rk, h))
			return -EINVAL;
		for (uint32_t w = 0; w < 4u; w++)
			d.hpow[0][w] = (uint32_t)h[4 * w] << 24 | (uint32_t)h[4 * w + 1] << 16 |
				       (uint32_t)h[4 * w + 2] << 8 | h[4 * w + 3];
		for (uint32_t k = 1; k < ESP_NPOW; k++)
			esp_gf_mul(d.hpow[k - 1u], d.hpow[0], d.hpow[k]);
		d.nr = sa->key_len / 4u + 6u;
		d.salt = (uint32_t)sa->salt[0] << 24 | (uint32_t)sa->salt[1] << 16 |
			 (uint32_t)sa->salt[2] << 8 | sa->salt[3];
		d.spi = sa->spi;
		d.flags = ESP_SA_VALID | (sa->df ? ESP_SA_DF : 0u) |
			  (sa->copy_dscp ? ESP_SA_COPY_DSCP : 0u) | (sa->copy_df ? ESP_SA_COPY_DF : 0u);
		d.tun_src = (uint32_t)sa->tun_src[0] << 24 | (uint32_t)sa->tun_src[1] << 16 |
			    (uint32_t)sa->tun_src[2] << 8 | sa->tun_src[3];
		d.tun_dst = (uint32_t)sa->tun_dst[0] << 24 | (uint32_t)sa->tun_dst[1] << 16 |
			    (uint32_t)sa->tun_dst[2] << 8 | sa->tun_dst[3];
		d.ttl_dscp = sa->ttl | (uint32_t)(sa->dscp & 0x3Fu) << 8;
		d.mtu = sa->mtu;
	}
	odpg_ctx_t *c = e->ctx;

	hipSetDevice(c->device);
	/* synchronous on the context stream: after the calls before it, before the
	 * calls after it */
	if (odpg_memcpy_h2d(c, e->sas + index, &d, sizeof(d)))
		return -EIO;
	if (e->a.next_seq && odpg_memcpy_h2d(c, e->a.next_seq + index, &one, sizeof(one)))
		return -EIO;
	return 0;
}

int odpg_esp(odpg_esp_t *e, const odpg_esp_src_t *src, const odpg_esp_dst_t *dst)
{
	if (!e || !src || !dst || !dst->frames || !dst->status || !dst->seq || !dst->total ||
	    (!dst->desc && dst->max_out) || (!src->frames && src->num) ||
	    (((uintptr_t)src->frames | (uintptr_t)dst->frames) & 15u) ||
	    (((uintptr_t)src->sa | (uintptr_t)src->l3_offset) & 1u) || src->num > e->max_pkts ||
	    (!src->desc && (!src->stride || (src->stride & 15u))) || dst->capacity > (1ull << 32))
		return -EINVAL;
	odpg_ctx_t *c = e->ctx;
	odpg_esp_args a = e->a;

	a.src = *src;
	a.dst = *dst;
	hipSetDevice(c->device);
	std::lock_guard<std::mutex> lk(c->lock);

	return odpg_launch_esp(&a, ctx_stream_locked(c));
}

static int ensure_ws(odpg_ctx_t *c, size_t bytes)
{
	if (c->ws_bytes >= bytes)
		return 0;
	if (c->ws) {
		HIPCHK(hipStreamSynchronize(ctx_stream_locked(c)));
		HIPCHK(hipFree(c->ws));
		c->ws = nullptr;
		c->ws_bytes = 0;
	}
	HIPCHK(hipMalloc(&c->ws, bytes));
	c->ws_bytes = bytes;
	return 0;
}

static int validate_batch(const odpg_batch_t *b)
{
	if (!b)
		return -EINVAL;
	if (b->num && !b->frames)
		return -EINVAL;
	if (!b->desc && (b->stride == 0 || (b->stride & 15u)))
		return -EINVAL;
	if (b->layer > 4)
		return -EINVAL;
	return 0;
}

/* one launch on lane `lane` (0: the context stream) */
static int classify_on(odpg_ctx_t *c, int lane, const odpg_table_t *t,
		       const odpg_batch_t *b, const odpg_result_t *r, void *ws)
{
	hipStream_t s = lane ? c->lane1 : c->stream;
	odpg_launch_args a;
	const dtable_hdr_t &h = t->hdr;
	uint32_t grid = odpg_launch_grid(b->num);
	bool cos_stats = r->stats && (h.flags & TBL_ANY_STATS);

	memset(&a, 0, sizeof(a));
	a.frames = b->frames;
	a.desc = b->desc;
	a.stride = b->stride;
	a.num = b->num;
	a.opt = b->pktin_opt;
	a.layer = b->layer;
	a.classify = b->classify;
	a.terms = (const dterm_t *)((const uint8_t *)t->dblob + h.term_off);
	a.pmrs = (const dpmr_t *)((const uint8_t *)t->dblob + h.pmr_off);
	a.coses = (const dcos_t *)((const uint8_t *)t->dblob + h.cos_off);
	a.num_cos = h.num_cos;
	a.default_cos = h.default_cos;
	a.error_cos = h.error_cos;
	a.tbl_flags = h.flags;
	a.num_pmr = h.num_pmr;
	a.slot_mask = h.slot_mask;
	a.slots = (const dslot_t *)((const uint8_t *)t->dblob + h.slot_off);
	a.simple = (const dsimple_t *)((const uint8_t *)t->dblob + h.simple_off);
	a.runs = (const drun_t *)((const uint8_t *)t->dblob + h.run_off);
	a.num_runs = h.num_runs;
	a.hgroups = (const dhgroup_t *)((const uint8_t *)t->dblob + h.hgroup_off);
	a.num_hgroups = h.num_hgroups;
	a.hents = (const dhent_t *)((const uint8_t *)t->dblob + h.hent_off);
	a.num_hent = h.num_hent;
	a.cinfo = (const uint2_t *)((const uint8_t *)t->dblob + h.cinfo_off);
	a.pinfo = (const uint32_t *)((const uint8_t *)t->dblob + h.pinfo_off);
	a.wgroups = (const dhgroup_t *)((const uint8_t *)t->dblob + h.wgroup_off);
	a.num_wgroups = h.num_wgroups;
	a.wents = (const dwent_t *)((const uint8_t *)t->dblob + h.went_off);
	a.num_went = h.num_went;
	a.mgroups = (const dmgroup_t *)((const uint8_t *)t->dblob + h.mgroup_off);
	a.num_mgroups = h.num_mgroups;
	a.ments = (const dment_t *)((const uint8_t *)t->dblob + h.ment_off);
	a.num_ment = h.num_ment;
	a.pinfo2 = (const uint2_t *)((const uint8_t *)t->dblob + h.pinfo2_off);
	a.cgroups = (const dmgroup_t *)((const uint8_t *)t->dblob + h.cgroup_off);
	a.num_cgroups = h.num_cgroups;
	a.cents = (const dwent_t *)((const uint8_t *)t->dblob + h.cent_off);
	a.num_cent = h.num_cent;
	a.pinfo3 = (const uint2_t *)((const uint8_t *)t->dblob + h.pinfo3_off);
	a.pinfo4 = (const uint32_t *)((const uint8_t *)t->dblob + h.pinfo4_off);
	a.def_cgmask = h.def_cgmask;
	a.xcos = (const uint2_t *)((const uint8_t *)t->dblob + h.xcos_off);
	a.xlist = (const uint32_t *)((const uint8_t *)t->dblob + h.xlist_off);
	a.num_xlist = h.num_xlist;
	a.num_xwords = h.num_xwords;
	a.xm = (const uint32_t *)((const uint8_t *)t->dblob + h.xm_off);
	a.num_xment = h.num_xment;
	a.xm_slot_bytes = h.xm_slot_bytes;
	a.num_xflat = h.num_xflat;
	a.xm_nw = h.xm_nw;
	a.xm_nbits = h.xm_nbits;
	a.xm_ngroups = h.xm_ngroups;
	a.xm_kx = h.xm_kx;
	{
		/* start state of cls_select_cos (odp_classification.c:1669-1701)
		 * for the lean kernel, as classify.hip derives it per packet */
		const dcos_t *hc = (const dcos_t *)(t->blob.data() + h.cos_off);
		const int32_t dc = h.default_cos, ec = h.error_cos;
		const bool dvalid = dc >= 0 && (uint32_t)dc < h.num_cos && hc[dc].valid;

		a.l64_err_cos = ec < 0 ? ODPG_COS_NONE : (uint32_t)ec;
		a.l64_err_act = ec >= 0 && (uint32_t)ec < h.num_cos ? hc[ec].action : 0u;
		a.l64_def_cos = dc < 0 ? ODPG_COS_NONE : (uint32_t)dc;
		a.l64_def_act = dc >= 0 && (uint32_t)dc < h.num_cos ? hc[dc].action : 0u;
		a.l64_def_rules = dvalid && hc[dc].nrule;
		a.l64_def_ci = dvalid && hc[dc].nrule ?
			       (hc[dc].rule_start & 0xffu) | ((uint32_t)(hc[dc].nrule & 0xffu) << 8) : 0u;
		const uint64_t dm = dvalid && hc[dc].nrule && hc[dc].rule_start < 64u ?
				    (hc[dc].nrule >= 64u ? ~0ull : ((1ull << hc[dc].nrule) - 1ull))
				    << hc[dc].rule_start : 0ull;

		a.l64_depth = t->depth;
		a.l64_def_mlo = (uint32_t)dm;
		a.l64_def_mhi = (uint32_t)(dm >> 32);
	}
	a.mode = c->kernel_mode;
	a.out = r->out;
	a.mark = r->mark;
	a.meta = r->meta;
	a.stats = r->stats;
	if (r->counters) {
		odpg_counters_t *k = r->counters;

		/* the lane's own rows: launches of a lane are stream-ordered */
		a.cnt.row = k->drows + (size_t)lane * k->rows * k->words;
		a.cnt.qcol = k->dqcol;
		a.cnt.words = k->words;
		a.cnt.rows = k->rows;
		a.cnt.ncos = k->ncos;
		a.cnt.ncols = k->ncols;
		a.cnt.cos = k->any_cos;
	} else if (r->stats && !cos_stats) {
		/* pktio counters only: workgroups add straight into them */
		a.pk_partial = r->stats;
		a.pk_atomic = 1u;
		a.sred = c->sred;
	} else if (r->stats) {
		a.pk_partial = (uint64_t *)ws;
		a.cos_partial = (uint32_t *)((uint8_t *)ws + (size_t)grid * 32u);
	}
	return odpg_launch_classify(&a, s);
}

static void free_stage(odpg_ctx_t *c)
{
	for (int k = 0; k < NSTAGE; k++) {
		Stage &B = c->stage[k];

		hipFree(B.frames);
		hipFree(B.desc);
		hipFree(B.out);
		hipFree(B.mark);
		hipFree(B.meta);
		if (B.hdesc)
			hipHostFree(B.hdesc);
		B.frames = nullptr;
		B.desc = nullptr;
		B.out = nullptr;
		B.mark = nullptr;
		B.meta = nullptr;
		B.hdesc = nullptr;
	}
	c->stage_span = 0;
	c->stage_chunk = 0;
	c->stage_flags = 0;
}

/* grow-only staging for odpg_classify_host */
static int ensure_stage(odpg_ctx_t *c, size_t span, uint32_t chunk, bool desc, bool mark,
			bool meta, uint32_t nstats)
{
	const uint32_t want = (desc ? 1u : 0u) | (mark ? 2u : 0u) | (meta ? 4u : 0u);

	if (c->stage_span < span + 16 || c->stage_chunk < chunk ||
	    (c->stage_flags & want) != want) {
		HIPCHK(hipStreamSynchronize(ctx_stream_locked(c)));
		HIPCHK(hipStreamSynchronize(c->copy_stream));
		const size_t nspan = span + 16 > c->stage_span ? span + 16 : c->stage_span;
		const uint32_t nchunk = chunk > c->stage_chunk ? chunk : c->stage_chunk;
		const uint32_t flags = want | c->stage_flags;

		free_stage(c);
		for (int k = 0; k < NSTAGE; k++) {
			Stage &B = c->stage[k];

			if (hipMalloc(&B.frames, nspan) != hipSuccess ||
			    hipMalloc(&B.out, (size_t)nchunk * sizeof(odpg_out_t)) != hipSuccess ||
			    ((flags & 1u) && (hipMalloc(&B.desc, (size_t)nchunk * sizeof(odpg_desc_t)) != hipSuccess ||
					      hipHostMalloc(&B.hdesc, (size_t)nchunk * sizeof(odpg_desc_t),
							    hipHostMallocDefault) != hipSuccess)) ||
			    ((flags & 2u) && hipMalloc(&B.mark, (size_t)nchunk * 2u) != hipSuccess) ||
			    ((flags & 4u) && hipMalloc(&B.meta, (size_t)nchunk * sizeof(odpg_meta_t)) != hipSuccess)) {
				free_stage(c);
				return -ENOMEM;
			}
		}
		c->stage_span = nspan;
		c->stage_chunk = nchunk;
		c->stage_flags = flags;
	}
	if (nstats > c->stage_nstats) {
		HIPCHK(hipStreamSynchronize(ctx_stream_locked(c)));
		hipFree(c->stage_stats);
		c->stage_stats = nullptr;
		c->stage_nstats = 0;
		if (hipMalloc(&c->stage_stats, nstats * 8u) != hipSuccess)
			return -ENOMEM;
		c->stage_nstats = nstats;
	}
	return 0;
}

static size_t ws_need(const odpg_table_t *t, uint32_t num, bool stats)
{
	if (!stats)
		return 0;
	if (!(t->hdr.flags & TBL_ANY_STATS))
		return 0;   /* pktio counters only: added in place */
	uint32_t grid = odpg_launch_grid(num);

	return (size_t)grid * 32u + (size_t)grid * t->hdr.num_cos * 4u;
}

/* a counters object serves launches on its own context (its rows are
 * updated with plain read-modify-writes, stream-ordered) and tables of its
 * layout; not together with the caller's stats block */
static int check_counters(const odpg_ctx_t *c, const odpg_table_t *t, const odpg_result_t *r)
{
	const odpg_counters_t *k = r->counters;

	if (!k)
		return 0;
	if (r->stats || k->ctx != c || k->qsig != t->qsig || k->ncos != t->hdr.num_cos)
		return -EINVAL;
	return 0;
}

int odpg_classify(odpg_ctx_t *c, const odpg_table_t *t, const odpg_batch_t *b,
		  const odpg_result_t *r)
{
	int rc;

	if (!c || !t || !r || (b && b->num && !r->out))
		return -EINVAL;
	if ((rc = validate_batch(b)))
		return rc;
	if (t->device != c->device)
		return -EXDEV;
	if ((rc = check_counters(c, t, r)))
		return rc;
	if (b->num == 0)
		return 0;
	std::lock_guard<std::mutex> g(c->lock);

	hipSetDevice(c->device);
	if ((rc = ensure_ws(c, ws_need(t, b->num, r->stats != nullptr))))
		return rc;
	if (r->stats || (r->counters && r->counters->sets != 2) || c->ls.lanes != 2) {
		/* stats launches share the context's scratch, and counted launches
		 * add into workgroup-owned rows with plain read-modify-writes: with
		 * one set of rows they stay in order on the context stream */
		ctx_stream_locked(c);
		return classify_on(c, 0, t, b, r, c->ws);
	}
	/* verdict-only, or counted into the lane's own set of rows: the next lane,
	 * behind whatever on the other lane touches the same bytes (lanes.h).
	 * Descriptor batches bound their frame bytes by the descriptor format
	 * (32-bit offset + 32-bit length) */
	const uintptr_t f = (uintptr_t)b->frames, o = (uintptr_t)r->out;
	lane_access acc = {};
	lane_act acts[LANE_MAX_ACTS];
	int n;

	acc.rd[0] = {f, f + (b->desc ? (uintptr_t)2 << 32 : (uintptr_t)b->num * b->stride)};
	if (b->desc)
		acc.rd[1] = {(uintptr_t)b->desc, (uintptr_t)b->desc + (uintptr_t)b->num * sizeof(odpg_desc_t)};
	acc.wr[0] = {o, o + (uintptr_t)b->num * sizeof(odpg_out_t)};
	if (r->mark)
		acc.wr[1] = {(uintptr_t)r->mark, (uintptr_t)r->mark + (uintptr_t)b->num * 2u};
	if (r->meta)
		acc.wr[2] = {(uintptr_t)r->meta, (uintptr_t)r->meta + (uintptr_t)b->num * sizeof(odpg_meta_t)};
	const int lane = lane_launch(&c->ls, &acc, acts, &n);

	if (lane_apply(c, acts, n))
		return -EIO;
	return classify_on(c, lane, t, b, r, c->ws);
}

/* Host-buffer path: frames/desc/results in host memory (pinned is fastest).
 * Two device buffer sets alternate between the copy stream (H2D) and the
 * compute stream (kernel + D2H). */
int odpg_classify_host(odpg_ctx_t *c, const odpg_table_t *t, const odpg_batch_t *b,
		       const odpg_result_t *r, uint32_t chunk)
{
	int rc;

	if (!c || !t || !r || (b && b->num && !r->out))
		return -EINVAL;
	if ((rc = validate_batch(b)))
		return rc;
	if (t->device != c->device)
		return -EXDEV;
	if ((rc = check_counters(c, t, r)))
		return rc;
	if (b->num == 0)
		return 0;
	if (chunk == 0)
		chunk = 1u << 18;
	if (chunk > b->num)
		chunk = b->num;
	std::lock_guard<std::mutex> g(c->lock);

	hipSetDevice(c->device);
	/* the lock is held to the end: no launch moves to the other lane meanwhile */
	hipStream_t cs = ctx_stream_locked(c);

	/* size the frame staging buffers */
	size_t max_span = 0;
	uint32_t nchunks = (b->num + chunk - 1) / chunk;
	std::vector<size_t> span_lo(nchunks), span_hi(nchunks);

	for (uint32_t k = 0; k < nchunks; k++) {
		uint32_t first = k * chunk, n = b->num - first < chunk ? b->num - first : chunk;
		size_t lo, hi;

		if (b->desc) {
			lo = (size_t)-1;
			hi = 0;
			for (uint32_t j = first; j < first + n; j++) {
				size_t o = b->desc[j].offset, e = o + b->desc[j].len;

				if (o & 15u)
					return -EINVAL;
				lo = o < lo ? o : lo;
				e = (e + 15u) & ~(size_t)15u;
				hi = e > hi ? e : hi;
			}
		} else {
			lo = (size_t)first * b->stride;
			hi = lo + (size_t)n * b->stride;
		}
		span_lo[k] = lo;
		span_hi[k] = hi;
		if (hi - lo > max_span)
			max_span = hi - lo;
	}

	uint32_t nstats = ODPG_STATS_WORDS(t->hdr.num_cos);
	int err = 0;

	if ((err = ensure_stage(c, max_span, chunk, b->desc != nullptr, r->mark != nullptr,
				r->meta != nullptr, r->stats ? nstats : 0u)))
		return err;
	if (r->stats && hipMemsetAsync(c->stage_stats, 0, nstats * 8u, cs) != hipSuccess)
		return -EIO;
	err = ensure_ws(c, ws_need(t, chunk, r->stats != nullptr));

	for (uint32_t k = 0; k < nchunks && !err; k++) {
		Stage &B = c->stage[k % NSTAGE];
		uint32_t first = k * chunk, n = b->num - first < chunk ? b->num - first : chunk;
		size_t lo = span_lo[k], bytes = span_hi[k] - span_lo[k];

		/* buffer reuse: the copy stream waits until the chunk that used this
		 * stage has been classified and its results copied back */
		if (k >= NSTAGE && hipStreamWaitEvent(c->copy_stream, B.compute_done, 0) != hipSuccess) {
			err = -EIO;
			break;
		}
		if (hipMemcpyAsync(B.frames, b->frames + lo, bytes, hipMemcpyHostToDevice,
				   c->copy_stream) != hipSuccess) {
			err = -EIO;
			break;
		}
		if (b->desc) {
			/* chunk-relative descriptors, staged through a pinned buffer
			 * the host rewrites once the stage's previous chunk is done */
			if (k >= NSTAGE)
				hipEventSynchronize(B.compute_done);
			for (uint32_t j = 0; j < n; j++) {
				B.hdesc[j].offset = (uint32_t)(b->desc[first + j].offset - lo);
				B.hdesc[j].len = b->desc[first + j].len;
			}
			if (hipMemcpyAsync(B.desc, B.hdesc, (size_t)n * sizeof(odpg_desc_t),
					   hipMemcpyHostToDevice, c->copy_stream) != hipSuccess) {
				err = -EIO;
				break;
			}
		}
		hipEventRecord(B.h2d_done, c->copy_stream);
		hipStreamWaitEvent(cs, B.h2d_done, 0);

		odpg_batch_t cb = *b;
		odpg_result_t cr;

		cb.frames = B.frames;
		cb.desc = b->desc ? B.desc : nullptr;
		cb.num = n;
		cr.out = B.out;
		cr.mark = r->mark ? B.mark : nullptr;
		cr.meta = r->meta ? B.meta : nullptr;
		cr.stats = r->stats ? c->stage_stats : nullptr;
		cr.counters = r->counters;
		if (classify_on(c, 0, t, &cb, &cr, c->ws)) {
			err = -EIO;
			break;
		}
		hipMemcpyAsync(r->out + first, B.out, (size_t)n * sizeof(odpg_out_t),
			       hipMemcpyDeviceToHost, cs);
		if (r->mark)
			hipMemcpyAsync(r->mark + first, B.mark, (size_t)n * 2u, hipMemcpyDeviceToHost,
				       cs);
		if (r->meta)
			hipMemcpyAsync(r->meta + first, B.meta, (size_t)n * sizeof(odpg_meta_t),
				       hipMemcpyDeviceToHost, cs);
		hipEventRecord(B.compute_done, cs);
	}
	if (!err && r->stats) {
		std::vector<uint64_t> hs(nstats);

		if (hipMemcpyAsync(hs.data(), c->stage_stats, nstats * 8u, hipMemcpyDeviceToHost,
				   cs) != hipSuccess ||
		    hipStreamSynchronize(cs) != hipSuccess)
			err = -EIO;
		else
			for (uint32_t k = 0; k < nstats; k++)
				r->stats[k] += hs[k];
	}
	if (hipStreamSynchronize(cs) != hipSuccess ||
	    hipStreamSynchronize(c->copy_stream) != hipSuccess)
		err = err ? err : -EIO;
	return err;
}

int odpg_dev_alloc(odpg_ctx_t *c, size_t bytes, void **ptr)
{
	if (!c || !ptr)
		return -EINVAL;
	hipSetDevice(c->device);
	if (hipMalloc(ptr, bytes ? bytes : 16) != hipSuccess)
		return -ENOMEM;
	return 0;
}

int odpg_dev_free(odpg_ctx_t *c, void *ptr)
{
	if (!c)
		return -EINVAL;
	hipSetDevice(c->device);
	ctx_stream(c);     /* a join, as for every call on the context */
	HIPCHK(hipFree(ptr));
	return 0;
}

int odpg_host_alloc_pinned(size_t bytes, void **ptr)
{
	if (!ptr)
		return -EINVAL;
	if (hipHostMalloc(ptr, bytes ? bytes : 16, hipHostMallocDefault) != hipSuccess)
		return -ENOMEM;
	return 0;
}

int odpg_host_device_ptr(void *host_ptr, void **dev_ptr)
{
	if (!host_ptr || !dev_ptr)
		return -EINVAL;
	if (hipHostGetDevicePointer(dev_ptr, host_ptr, 0) != hipSuccess)
		return -EINVAL;
	return 0;
}

int odpg_host_free_pinned(void *ptr)
{
	if (!ptr)
		return 0;
	HIPCHK(hipHostFree(ptr));
	return 0;
}

int odpg_memcpy_h2d(odpg_ctx_t *c, void *dst, const void *src, size_t bytes)
{
	if (!c)
		return -EINVAL;
	hipStream_t cs = ctx_stream(c);

	HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, cs));
	HIPCHK(hipStreamSynchronize(cs));
	return 0;
}

int odpg_memcpy_d2h(odpg_ctx_t *c, void *dst, const void *src, size_t bytes)
{
	if (!c)
		return -EINVAL;
	hipStream_t cs = ctx_stream(c);

	HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, cs));
	HIPCHK(hipStreamSynchronize(cs));
	return 0;
}

int odpg_memset_dev(odpg_ctx_t *c, void *dst, int value, size_t bytes)
{
	if (!c)
		return -EINVAL;
	HIPCHK(hipMemsetAsync(dst, value, bytes, ctx_stream(c)));
	return 0;
}

int odpg_event_record(odpg_ctx_t *c, int slot)
{
	if (!c || slot < 0 || slot >= NUM_EVENTS)
		return -EINVAL;
	HIPCHK(hipEventRecord(c->ev[slot], ctx_stream(c)));
	return 0;
}

struct odpg_fence_s {
	hipEvent_t ev;
	int device;
	odpg_ctx_t *ctx;   /* referenced: any destroy order (odpg.h) */
};

int odpg_fence_create(odpg_ctx_t *c, odpg_fence_t **fence)
{
	if (!c || !fence)
		return -EINVAL;
	odpg_fence_t *f = new (std::nothrow) odpg_fence_t;

	if (!f)
		return -ENOMEM;
	f->device = c->device;
	f->ctx = c;
	hipSetDevice(c->device);
	if (hipEventCreateWithFlags(&f->ev, hipEventDisableTiming) != hipSuccess) {
		delete f;
		return -EIO;
	}
	odpg_ctx_ref(c);
	*fence = f;
	return 0;
}

int odpg_fence_record(odpg_ctx_t *c, odpg_fence_t *f)
{
	if (!c || !f || f->device != c->device)
		return -EINVAL;
	HIPCHK(hipEventRecord(f->ev, ctx_stream(c)));
	return 0;
}

int odpg_fence_query(odpg_fence_t *f)
{
	if (!f)
		return -EINVAL;
	const hipError_t e = hipEventQuery(f->ev);

	return e == hipSuccess ? 1 : e == hipErrorNotReady ? 0 : -EIO;
}

int odpg_fence_wait(odpg_fence_t *f)
{
	if (!f)
		return -EINVAL;
	HIPCHK(hipEventSynchronize(f->ev));
	return 0;
}

void odpg_fence_destroy(odpg_fence_t *f)
{
	if (!f)
		return;
	hipSetDevice(f->device);
	hipEventDestroy(f->ev);
	odpg_ctx_unref(f->ctx);
	delete f;
}

int odpg_event_elapsed_ms(odpg_ctx_t *c, int a, int b, float *ms)
{
	if (!c || !ms || a < 0 || b < 0 || a >= NUM_EVENTS || b >= NUM_EVENTS)
		return -EINVAL;
	HIPCHK(hipEventSynchronize(c->ev[b]));
	HIPCHK(hipEventElapsedTime(ms, c->ev[a], c->ev[b]));
	return 0;
}

} /* extern "C" */
