/* SPDX-License-Identifier: BSD-3-Clause
 *
 * Launch lanes: the bookkeeping that lets consecutive odpg_classify launches
 * of one context (verdict-only, or counted into per-lane counter rows) run on
 * two streams ("lanes") while results stay what call order gives. Plain C
 * without HIP: runtime.hip carries out the actions decided here with HIP
 * events, tests/c/lanes_model.cpp and lanes_join_model.cpp carry them out in
 * a happens-before model.
 *
 * Lane 0 is the context stream, lane 1 the second stream. Each lane keeps a
 * bounded ring of the byte ranges read and written by those of its launches
 * the other lane is not yet ordered after. Events cost several microseconds
 * of host time each (measured: one record and one wait per two launches
 * tripled the enqueue time), so the steady state records none:
 *   - a launch that conflicts with recorded launches of one lane only runs
 *     on that lane, where stream order is the dependency (a receive loop
 *     over a ring of buffer sets reuses a set on the lane that used it
 *     last);
 *   - a launch without conflicts takes the lane the previous launch did
 *     not;
 *   - a recorded launch whose ranges a later launch of the same lane covers
 *     is forgotten: whatever conflicts with it conflicts with the later one.
 * An event is recorded only when a launch conflicts with both lanes, when a
 * ring is full, and at joins: the lane's launches since its last event form
 * an epoch, closed by recording one event behind them, and the other lane
 * waits for the event of the newest epoch it needs.
 *
 * Every other use of the context stream is a join (lane_join): lane 0 waits
 * for lane 1's recorded launches, and the next launch on lane 1 first waits
 * for lane 0 (`dirty`). A join leaves lane 0 as the next lane, so a caller
 * that alternates launch and join stays on lane 0 and never records an
 * event; while `dirty` is set lane 0's ring is only a hint for the choice of
 * lane (lane 1 waits for all of lane 0 anyway) and drops its oldest entry
 * when full. Lane 1 has to wait for a point of lane 0 behind the join's work
 * and, to stay unordered with the launch that follows the join, in front of
 * that launch. No event can be recorded there after the fact, so when the
 * join itself had to wait for lane 1 (the caller does overlap launches:
 * `fork`) the first launch after it records lane 0's event in front of
 * itself; otherwise the event is recorded when lane 1 is first used, behind
 * the launches lane 0 has taken since.
 *
 * The join state (`dirty`, `fork`, `join_epoch`) and what moves it:
 *
 *   call                         | before          | actions decided           | after
 *   -----------------------------+-----------------+---------------------------+----------------
 *   lane_join, lane 1 ring empty | any             | none                      | dirty 1
 *   lane_join, lane 1 ring used  | any             | lane 0 waits for lane 1   | dirty 1, fork 1
 *   launch on lane 0             | dirty 1, fork 1 | record E on lane 0        | dirty 2, fork 0,
 *                                |                 |                           | join_epoch = E
 *   launch on lane 0             | otherwise       | none for the join         | fork 0
 *   launch on lane 1             | dirty 1         | record on lane 0, lane 1  | dirty 0, lane 0
 *                                |                 | waits for it              | ring emptied
 *   launch on lane 1             | dirty 2         | lane 1 waits for E        | dirty 0, lane 0
 *                                |                 |                           | ring cut up to E
 *   launch on lane 1             | dirty 0         | none for the join         | unchanged
 *
 * Invariants: dirty != 0 exactly when lane 0 holds work (a join's, or
 * launches before it) lane 1 is not ordered after; dirty == 2 implies that
 * event join_epoch of lane 0 was recorded behind the last join and in front
 * of every lane-0 launch since (a later record into the same slot is a later
 * point of the same stream, so waiting for the slot still orders after E);
 * fork is set by a join and cleared by the first two-lane launch after it,
 * which is always on lane 0 (lane 1's ring is empty after a join and `next`
 * is 0; with one lane lane_launch decides nothing and leaves it). While
 * dirty == 1 every record of lane 0's ring, and while dirty == 2 those of
 * epochs up to join_epoch, are covered by the wait lane 1 does before its next
 * launch, so a full ring may drop them without an event. lane_set is a join
 * that also empties lane 0's ring.
 */
#ifndef ODPG_LANES_H_
#define ODPG_LANES_H_

#include <stdint.h>
#include <string.h>

#define LANE_RING   8    /* recorded launches per lane */
#define LANE_NEV    8    /* epoch events per lane */
#define LANE_MAX_ACTS 12 /* more than one call decides (at most 11) */

typedef struct lane_span {
	uintptr_t lo, hi;    /* [lo, hi), lo == hi: nothing */
} lane_span;

typedef struct lane_access {
	lane_span rd[2];     /* frames, desc */
	lane_span wr[3];     /* out, mark, meta */
} lane_access;

enum {
	LANE_RECORD = 1,     /* record event `slot` of `lane` on `lane` */
	LANE_WAIT = 2        /* the lane other than `lane` waits for event `slot` of `lane` */
};

typedef struct lane_act {
	uint8_t op, lane, slot;
} lane_act;

typedef struct lane_ring {
	lane_access a[LANE_RING];
	uint32_t epoch_of[LANE_RING];   /* oldest first */
	uint32_t n;
	uint32_t epoch;                 /* the open epoch */
	uint32_t open_n;                /* launches in it */
} lane_ring;

typedef struct lane_state {
	lane_ring r[2];
	int lanes;           /* 2: eligible launches alternate; 1: all on lane 0 */
	int next;            /* lane of the next eligible launch */
	int dirty;           /* lane 0 has work lane 1 is not ordered after: 1 up to an
			      * event yet to record, 2 up to the event of join_epoch */
	int fork;            /* lane 1 had launches at a join since lane 0's last launch */
	uint32_t join_epoch; /* dirty == 2: lane 0's epoch closed behind the join */
} lane_state;

static inline void lane_init(lane_state *s, int lanes)
{
	memset(s, 0, sizeof(*s));
	s->lanes = lanes;
}

static inline int lane_span_hit(const lane_span *x, const lane_span *y)
{
	return x->lo < y->hi && y->lo < x->hi;
}

/* write / write, write / read or read / write on a common byte */
static inline int lane_conflict(const lane_access *x, const lane_access *y)
{
	for (int i = 0; i < 3; i++) {
		for (int j = 0; j < 3; j++)
			if (lane_span_hit(&x->wr[i], &y->wr[j]))
				return 1;
		for (int j = 0; j < 2; j++)
			if (lane_span_hit(&x->wr[i], &y->rd[j]) || lane_span_hit(&y->wr[i], &x->rd[j]))
				return 1;
	}
	return 0;
}

static inline void lane_act_add(lane_act *acts, int *n, int op, int lane, uint32_t epoch)
{
	acts[*n].op = (uint8_t)op;
	acts[*n].lane = (uint8_t)lane;
	acts[*n].slot = (uint8_t)(epoch % LANE_NEV);
	(*n)++;
}

/* forget the recorded launches of epochs up to `epoch` */
static inline void lane_drop(lane_ring *r, uint32_t epoch)
{
	uint32_t k = 0;

	while (k < r->n && r->epoch_of[k] <= epoch)
		k++;
	for (uint32_t i = k; i < r->n; i++) {
		r->a[i - k] = r->a[i];
		r->epoch_of[i - k] = r->epoch_of[i];
	}
	r->n -= k;
}

/* close lane l's open epoch: its event slot was last used LANE_NEV epochs
 * ago; recorded launches that still name that event retire first */
static inline void lane_close(lane_state *s, int l, lane_act *acts, int *n)
{
	lane_ring *r = &s->r[l];

	if (r->n && r->epoch >= LANE_NEV && r->epoch_of[0] <= r->epoch - LANE_NEV) {
		lane_act_add(acts, n, LANE_WAIT, l, r->epoch);
		lane_drop(r, r->epoch - LANE_NEV);
	}
	lane_act_add(acts, n, LANE_RECORD, l, r->epoch);
	r->epoch++;
	r->open_n = 0;
}

/* the other lane waits for every recorded launch of lane l up to epoch */
static inline void lane_wait_epoch(lane_state *s, int l, uint32_t epoch, lane_act *acts, int *n)
{
	lane_ring *r = &s->r[l];

	if (epoch == r->epoch)
		lane_close(s, l, acts, n);
	lane_act_add(acts, n, LANE_WAIT, l, epoch);
	lane_drop(r, epoch);
}

static inline int lane_span_in(const lane_span *x, const lane_span *y)
{
	return x->lo == x->hi || (y->lo <= x->lo && x->hi <= y->hi);
}

/* every read of x lies in a range y reads or writes, every write of x in a
 * range y writes: what conflicts with x conflicts with y */
static inline int lane_covers(const lane_access *y, const lane_access *x)
{
	for (int i = 0; i < 2; i++)
		if (!lane_span_in(&x->rd[i], &y->rd[0]) && !lane_span_in(&x->rd[i], &y->rd[1]) &&
		    !lane_span_in(&x->rd[i], &y->wr[0]) && !lane_span_in(&x->rd[i], &y->wr[1]) &&
		    !lane_span_in(&x->rd[i], &y->wr[2]))
			return 0;
	for (int i = 0; i < 3; i++)
		if (!lane_span_in(&x->wr[i], &y->wr[0]) && !lane_span_in(&x->wr[i], &y->wr[1]) &&
		    !lane_span_in(&x->wr[i], &y->wr[2]))
			return 0;
	return 1;
}

/* the newest recorded launch of ring r that conflicts with a, or -1 */
static inline int lane_newest_conflict(const lane_ring *r, const lane_access *a)
{
	for (uint32_t i = r->n; i-- > 0;)
		if (lane_conflict(a, &r->a[i]))
			return (int)i;
	return -1;
}

/* An eligible launch with accesses `a`: returns its lane and the actions to
 * carry out, in order, before it is enqueued there. */
static inline int lane_launch(lane_state *s, const lane_access *a, lane_act *acts, int *nacts)
{
	*nacts = 0;
	if (s->lanes != 2)
		return 0;
	const int c0 = lane_newest_conflict(&s->r[0], a), c1 = lane_newest_conflict(&s->r[1], a);
	const int l = (c0 >= 0) != (c1 >= 0) ? (c1 >= 0) : s->next, o = l ^ 1;
	lane_ring *r = &s->r[l], *ro = &s->r[o];

	s->next = o;
	if (l == 0 && s->fork) {
		/* the first launch after a join that found lane 1 busy: lane 1 will
		 * be used again, let it wait for the join and not for this launch */
		if (s->dirty == 1) {
			lane_close(s, 0, acts, nacts);
			s->join_epoch = s->r[0].epoch - 1u;
			s->dirty = 2;
		}
		s->fork = 0;
	}
	if (l == 1 && s->dirty == 2) {
		/* behind the join: that event is there already */
		lane_act_add(acts, nacts, LANE_WAIT, 0, s->join_epoch);
		lane_drop(&s->r[0], s->join_epoch);
		s->dirty = 0;
	} else if (l == 1 && s->dirty) {
		/* behind everything on the context stream */
		lane_close(s, 0, acts, nacts);
		lane_act_add(acts, nacts, LANE_WAIT, 0, s->r[0].epoch - 1u);
		s->r[0].n = 0;
		s->dirty = 0;
	}
	for (uint32_t i = ro->n; i-- > 0;)
		if (lane_conflict(a, &ro->a[i])) {
			lane_wait_epoch(s, o, ro->epoch_of[i], acts, nacts);
			break;
		}
	/* recorded launches of this lane the new one covers */
	uint32_t k = 0;

	for (uint32_t i = 0; i < r->n; i++)
		if (!lane_covers(a, &r->a[i])) {
			r->a[k] = r->a[i];
			r->epoch_of[k++] = r->epoch_of[i];
		}
	r->n = k;
	if (r->n == LANE_RING) {
		if (l == 0 && (s->dirty == 1 || (s->dirty == 2 && r->epoch_of[0] <= s->join_epoch))) {
			/* lane 1 waits for the oldest before its next launch anyway */
			for (uint32_t i = 1; i < r->n; i++) {
				r->a[i - 1u] = r->a[i];
				r->epoch_of[i - 1u] = r->epoch_of[i];
			}
			r->n--;
		} else {
			lane_wait_epoch(s, l, r->epoch_of[0], acts, nacts);
		}
	}
	r->a[r->n] = *a;
	r->epoch_of[r->n] = r->epoch;
	r->n++;
	r->open_n++;
	return l;
}

/* Before any other use of the context stream: lane 0 waits for lane 1's
 * recorded launches. The next launch takes lane 0. */
static inline void lane_join(lane_state *s, lane_act *acts, int *nacts)
{
	lane_ring *r = &s->r[1];

	*nacts = 0;
	if (r->n) {
		lane_wait_epoch(s, 1, r->epoch_of[r->n - 1u], acts, nacts);
		s->fork = 1;
	}
	s->dirty = 1;
	s->next = 0;
}

/* one lane (all launches on lane 0, after a join) or two */
static inline void lane_set(lane_state *s, int lanes, lane_act *acts, int *nacts)
{
	lane_join(s, acts, nacts);
	s->r[0].n = 0;       /* lane 1 waits for lane 0 before its next launch (dirty) */
	s->lanes = lanes;
	s->next = 0;
}

#endif
