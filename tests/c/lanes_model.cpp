/* SPDX-License-Identifier: BSD-3-Clause
 *
 * The launch-lane bookkeeping (odp_amd/csrc/lanes.h) against a brute-force
 * happens-before model, no GPU: random sequences of verdict-only launches
 * (over a small pool of buffers, so that write / write, write / read and
 * read / read pairs all occur), joins (any other call on the context) and
 * lane switches go through lane_launch / lane_join / lane_set; the actions
 * they decide (record an event on a lane, make the other lane wait for it)
 * are carried out on vector clocks. Checked for every sequence:
 *   - every pair of conflicting launches is ordered, earlier before later;
 *   - a join is ordered after every earlier launch, and every later launch
 *     after the join;
 *   - a ring never holds more than LANE_RING launches, a call never decides
 *     more than LANE_MAX_ACTS actions;
 *   - launches that touch disjoint memory do overlap somewhere (the
 *     bookkeeping does not simply serialise everything).
 * And one fixed sequence, the receive loop over a ring of five buffer sets:
 * a launch is ordered after the one five calls back, four launches in five
 * stay unordered with the one before them, and no event is recorded after
 * the first round; over a ring of four sets every launch stays unordered
 * with the one before it.
 * Built with -fsanitize=address,undefined by tests/c/lanes_model.mk.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "../../odp_amd/csrc/lanes.h"

struct Clock {
	uint32_t c[2];
};

struct Op {
	int lane;          /* stream it was enqueued on */
	uint32_t idx;      /* its position on that stream (1-based) */
	Clock seen;        /* what it is ordered after */
	bool launch;       /* else a join (another call on the context stream) */
	lane_access a;
};

struct Model {
	Clock now[2] = {};                 /* per stream: what its next op is ordered after */
	Clock ev[2][LANE_NEV] = {};
	bool ev_set[2][LANE_NEV] = {};
	std::vector<Op> ops;

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
			} else if (acts[i].op == LANE_WAIT) {
				if (!ev_set[l][s])
					return -1;          /* a wait for an event never recorded */
				for (int k = 0; k < 2; k++)
					if (ev[l][s].c[k] > now[l ^ 1].c[k])
						now[l ^ 1].c[k] = ev[l][s].c[k];
			} else {
				return -1;
			}
		}
		return 0;
	}

	void enqueue(int lane, bool launch, const lane_access &a)
	{
		Op o;

		o.lane = lane;
		o.idx = ++now[lane].c[lane];
		o.seen = now[lane];
		o.launch = launch;
		o.a = a;
		ops.push_back(o);
	}
};

static bool before(const Op &x, const Op &y)
{
	return y.seen.c[x.lane] >= x.idx;
}

static uint64_t rng_state;
static uint32_t rnd(uint32_t n)
{
	rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
	return (uint32_t)(rng_state >> 33) % n;
}

static lane_span span(uintptr_t lo, uintptr_t bytes)
{
	return lane_span{lo, lo + bytes};
}

#define CHECK(x)                                                                        \
	do {                                                                            \
		if (!(x)) {                                                             \
			printf("FAIL seq %u: %s (line %d)\n", seq, #x, __LINE__);       \
			return 1;                                                       \
		}                                                                       \
	} while (0)

int main(int argc, char **argv)
{
	const uint32_t nseq = argc > 1 ? (uint32_t)atoi(argv[1]) : 4000u;
	uint64_t overlaps = 0, launches = 0;

	for (uint32_t seq = 0; seq < nseq; seq++) {
		rng_state = 0x9E3779B97F4A7C15ull ^ ((uint64_t)seq << 17);
		lane_state s;
		Model m;
		const uint32_t nops = 4u + rnd(60);
		const uint32_t nbuf = 1u + rnd(7);     /* few buffers: many conflicts */
		const uint32_t pjoin = rnd(4) ? rnd(20) : 50u;
		lane_act acts[LANE_MAX_ACTS + 4];
		int n;

		lane_init(&s, rnd(8) ? 2 : 1);
		for (uint32_t k = 0; k < nops; k++) {
			const uint32_t what = rnd(100);

			if (what < pjoin) {
				lane_join(&s, acts, &n);
				CHECK(m.apply(acts, n) == 0);
				m.enqueue(0, false, lane_access{});
			} else if (what < pjoin + 3u) {
				lane_set(&s, s.lanes == 2 ? 1 : 2, acts, &n);
				CHECK(m.apply(acts, n) == 0);
			} else {
				/* frames in [0x1000 ..), outs in [0x100000 ..), sometimes a
				 * mark / meta array, sometimes an out that overlaps another
				 * launch's out partly or aliases a frame buffer */
				lane_access a = {};
				const uintptr_t fb = 0x1000u + 0x1000u * rnd(nbuf);
				uintptr_t ob = 0x100000u + 0x1000u * rnd(nbuf) + 0x100u * rnd(3);

				if (rnd(16) == 0)
					ob = 0x1000u + 0x1000u * rnd(nbuf);
				a.rd[0] = {fb, fb + 0x400u + 0x400u * rnd(3)};
				if (rnd(4) == 0)
					a.rd[1] = span(0x200000u + 0x100u * rnd(nbuf), 0x80u + 0x80u * rnd(4));
				a.wr[0] = {ob, ob + 0x100u + 0x200u * rnd(4)};
				if (rnd(5) == 0)
					a.wr[1] = span(0x300000u + 0x100u * rnd(nbuf), 0x100u + 0x80u * rnd(4));
				if (rnd(7) == 0)
					a.wr[2] = span(0x400000u + 0x100u * rnd(nbuf), 0x100u + 0x80u * rnd(4));
				const int lane = lane_launch(&s, &a, acts, &n);

				CHECK(lane == 0 || (lane == 1 && s.lanes == 2));
				CHECK(m.apply(acts, n) == 0);
				m.enqueue(lane, true, a);
				launches++;
			}
			CHECK(s.r[0].n <= LANE_RING && s.r[1].n <= LANE_RING);
		}
		/* the brute-force check over every pair, in call order */
		for (size_t j = 0; j < m.ops.size(); j++)
			for (size_t i = 0; i < j; i++) {
				const Op &x = m.ops[i], &y = m.ops[j];
				const bool must = !x.launch || !y.launch || lane_conflict(&x.a, &y.a);

				if (must)
					CHECK(before(x, y));
				else if (!before(x, y))
					overlaps++;
			}
	}
	/* two lanes are worth something only if independent launches stay unordered */
	if (overlaps == 0) {
		printf("FAIL: no independent pair left unordered\n");
		return 1;
	}
	/* the receive loop: launch k reads frames k % nset and writes out k % nset */
	for (uint32_t nset = 4; nset <= 5; nset++) {
		const uint32_t seq = nseq, nl = 1000;
		lane_state s;
		Model m;
		lane_act acts[LANE_MAX_ACTS + 4];
		int n;
		uint32_t records = 0, free_of_prev = 0;

		lane_init(&s, 2);
		lane_join(&s, acts, &n);
		CHECK(m.apply(acts, n) == 0);
		for (uint32_t k = 0; k < nl; k++) {
			lane_access a = {};

			a.rd[0] = {0x1000u + 0x1000u * (k % nset), 0x2000u + 0x1000u * (k % nset)};
			a.wr[0] = {0x100000u + 0x1000u * (k % nset), 0x101000u + 0x1000u * (k % nset)};
			const int lane = lane_launch(&s, &a, acts, &n);

			CHECK(m.apply(acts, n) == 0);
			for (int i = 0; i < n; i++)
				records += k >= nset && acts[i].op == LANE_RECORD;
			m.enqueue(lane, true, a);
			if (k >= nset)
				CHECK(before(m.ops[k - nset], m.ops[k]));
			free_of_prev += k >= 1u && !before(m.ops[k - 1u], m.ops[k]);
			CHECK(s.r[0].n + s.r[1].n <= nset);
		}
		CHECK(records == 0);
		CHECK(free_of_prev >= (nset == 4 ? nl - 2u : nl * 4u / 5u - 2u));
		printf("ring of %u: %u launches, %u free of the one before, no event after the first round\n",
		       nset, nl, free_of_prev);
	}
	printf("PASS: %u sequences, %llu launches, %llu independent pairs left unordered\n", nseq,
	       (unsigned long long)launches, (unsigned long long)overlaps);
	return 0;
}
