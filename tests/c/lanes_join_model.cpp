/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Joins of the launch-lane bookkeeping (odp_amd/csrc/lanes.h), no GPU: the
 * actions lane_launch / lane_join / lane_set decide are carried out on vector
 * clocks, as in lanes_model.cpp. Three fixed call patterns:
 *   (a) launch, join, 1000 times, over disjoint buffers and over one buffer
 *       set: no LANE_RECORD action after the first iteration (events cost
 *       several microseconds of host time each), every launch ordered after
 *       the join before it and before the join after it;
 *   (b) launch, launch, join, 1000 times: the two launches of an iteration
 *       stay unordered with each other, the join is ordered after both, and
 *       both are ordered after the join before them;
 *   (c) after lane_set(.., 1) and lane_set(.., 2) the first launch takes
 *       lane 0.
 * Built with -fsanitize=address,undefined by tests/c/lanes_join_model.mk.
 */
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../odp_amd/csrc/lanes.h"

struct Clock {
	uint32_t c[2];
};

struct Op {
	int lane;          /* stream it was enqueued on */
	uint32_t idx;      /* its position on that stream (1-based) */
	Clock seen;        /* what it is ordered after */
};

struct Model {
	Clock now[2] = {};
	Clock ev[2][LANE_NEV] = {};
	bool ev_set[2][LANE_NEV] = {};
	uint32_t records = 0;

	int apply(const lane_act *acts, int n)
	{
		if (n > LANE_MAX_ACTS)
			return -1;
		for (int i = 0; i < n; i++) {
			const int l = acts[i].lane, s = acts[i].slot;

			if (l > 1 || s >= LANE_NEV)
				return -1;
			if (acts[i].op == LANE_RECORD) {
				ev[l][s] = now[l];
				ev_set[l][s] = true;
				records++;
			} else if (acts[i].op == LANE_WAIT) {
				if (!ev_set[l][s])
					return -1;
				for (int k = 0; k < 2; k++)
					if (ev[l][s].c[k] > now[l ^ 1].c[k])
						now[l ^ 1].c[k] = ev[l][s].c[k];
			} else {
				return -1;
			}
		}
		return 0;
	}

	Op enqueue(int lane)
	{
		Op o;

		o.lane = lane;
		o.idx = ++now[lane].c[lane];
		o.seen = now[lane];
		return o;
	}
};

static bool before(const Op &x, const Op &y)
{
	return y.seen.c[x.lane] >= x.idx;
}

/* buffer set k: frames and out of 4 KiB each */
static lane_access set_of(uint32_t k)
{
	lane_access a = {};

	a.rd[0] = {0x1000000u + 0x1000u * k, 0x1001000u + 0x1000u * k};
	a.wr[0] = {0x9000000u + 0x1000u * k, 0x9001000u + 0x1000u * k};
	return a;
}

#define CHECK(x)                                                                        \
	do {                                                                            \
		if (!(x)) {                                                             \
			printf("FAIL %s, iteration %u: %s (line %d)\n", what, it, #x, __LINE__); \
			return 1;                                                       \
		}                                                                       \
	} while (0)

static int launch(lane_state &s, Model &m, const lane_access &a, Op &o, int *lane = nullptr)
{
	lane_act acts[LANE_MAX_ACTS + 4];
	int n;
	const int l = lane_launch(&s, &a, acts, &n);

	if ((l != 0 && l != 1) || m.apply(acts, n))
		return -1;
	if (s.r[0].n > LANE_RING || s.r[1].n > LANE_RING)
		return -1;
	o = m.enqueue(l);
	if (lane)
		*lane = l;
	return 0;
}

static int join(lane_state &s, Model &m, Op &o)
{
	lane_act acts[LANE_MAX_ACTS + 4];
	int n;

	lane_join(&s, acts, &n);
	if (m.apply(acts, n))
		return -1;
	o = m.enqueue(0);
	return 0;
}

int main()
{
	const uint32_t iters = 1000;

	/* (a) launch, join */
	for (int same = 0; same < 2; same++) {
		const char *what = same ? "(a) one buffer set" : "(a) disjoint buffers";
		lane_state s;
		Model m;
		Op j = {}, l = {}, jn = {};
		uint32_t late_records = 0;

		lane_init(&s, 2);
		for (uint32_t it = 0; it < iters; it++) {
			const uint32_t r0 = m.records;
			int lane;

			CHECK(launch(s, m, set_of(same ? 0u : it), l, &lane) == 0);
			CHECK(lane == 0);
			if (it)
				CHECK(before(j, l));
			CHECK(join(s, m, jn) == 0);
			CHECK(before(l, jn));
			j = jn;
			if (it)
				late_records += m.records - r0;
			CHECK(late_records == 0);
		}
		printf("%s: %u iterations, %u events recorded\n", what, iters, m.records);
	}
	/* (b) launch, launch, join */
	for (int same = 0; same < 2; same++) {
		const char *what = same ? "(b) two buffer sets" : "(b) disjoint buffers";
		lane_state s;
		Model m;
		Op j = {}, l1 = {}, l2 = {}, jn = {};

		lane_init(&s, 2);
		for (uint32_t it = 0; it < iters; it++) {
			int a, b;

			CHECK(launch(s, m, set_of(same ? 0u : 2u * it), l1, &a) == 0);
			CHECK(launch(s, m, set_of(same ? 1u : 2u * it + 1u), l2, &b) == 0);
			CHECK(a == 0 && b == 1);
			CHECK(!before(l1, l2) && !before(l2, l1));
			if (it)
				CHECK(before(j, l1) && before(j, l2));
			CHECK(join(s, m, jn) == 0);
			CHECK(before(l1, jn) && before(l2, jn));
			j = jn;
		}
		printf("%s: %u iterations, %u events recorded\n", what, iters, m.records);
	}
	/* (c) one lane and back */
	{
		const char *what = "(c) lane_set";
		const uint32_t it = 0;
		lane_state s;
		Model m;
		lane_act acts[LANE_MAX_ACTS + 4];
		Op l = {}, l2 = {};
		int n, lane;

		lane_init(&s, 2);
		/* leave the next launch due on lane 1 */
		CHECK(launch(s, m, set_of(0), l, &lane) == 0 && lane == 0);
		lane_set(&s, 1, acts, &n);
		CHECK(m.apply(acts, n) == 0);
		CHECK(launch(s, m, set_of(1), l, &lane) == 0 && lane == 0);
		lane_set(&s, 2, acts, &n);
		CHECK(m.apply(acts, n) == 0);
		CHECK(launch(s, m, set_of(2), l, &lane) == 0);
		CHECK(lane == 0);
		CHECK(launch(s, m, set_of(3), l2, &lane) == 0);
		CHECK(lane == 1);
		printf("%s: first launch on lane 0\n", what);
	}
	printf("PASS: joins\n");
	return 0;
}
