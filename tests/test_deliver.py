"""Device-side CoS queue delivery lists (include/odpg_deliver.h).

odpg_deliver() is a stable partition of the packet indices by destination
bucket. Reference: numpy on the same verdict words (the bucket rule of the
header, a stable argsort, a cumulative bincount); integer results, compared
exactly. T = the tile one workgroup ranks; sizes sit on the wave edge (64),
the tile edge and over several tiles."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import ALL_CHKSUM, expected_counters
from odp_amd import _lib as L
from odp_amd import gen

T = L.DELIVER_TILE
MIXED = (1, 7, 3, 32, 1, 1)          # queues per CoS; the last CoS drops
SENTINELS = (L.ODPG_COS_NONE, L.ODPG_COS_PDROP, L.ODPG_COS_LOOP, L.ODPG_COS_NOCLS)


def make_plan(cls, ctx, kind, max_pkts):
    """(table, plan, rules) of a table kind: "mixed" (MIXED, one pass), "wide"
    (80 CoS of 32 queues: B = 2562, two passes), "c4" (B = 1027, the widest
    one-pass table) or "c2"."""
    if kind in ("wide", "c4"):
        assert cls.set_limits(2048, 2048, 128) == 0
    p = cls.loop_pktio(pktin=ALL_CHKSUM)
    if kind == "c4":
        gen.build_c4_rules(cls, p)
    elif kind == "c2":
        gen.build_c2_rules(cls, p)
    else:
        queues = MIXED if kind == "mixed" else (1,) + (32,) * 80
        default = cls.cos_create("c0", queue=cls.queue(0))
        assert cls.default_cos_set(p, default) == 0
        for i, nq in enumerate(queues[1:], 1):
            drop = kind == "mixed" and i == len(queues) - 1
            c = cls.cos_create(f"c{i}", queue=cls.queue(i), num_queue=nq, hash_proto=cls.HASH_IPV4,
                               action=cls.COS_ACTION_DROP if drop else cls.COS_ACTION_ENQUEUE)
            # referenced from the default CoS, so the compiled table keeps it
            assert c and cls.pmr_create([cls.Term(cls.PMR_UDP_DPORT, gen.be_bytes(i, 2),
                                                  b"\xff\xff")], default, c)
    assert cls.pktio_start(p) == 0
    rules = cls.pktio_rules(p)
    tbl = ctx.table(rules)
    return tbl, ctx.deliver(tbl, max_pkts), rules


def expected(plan, words):
    """(bucket, order, offsets) of `words`, the layout taken from the plan."""
    nc, B = plan.num_cos, plan.num_buckets
    qb = np.array([plan.queue_base(c) for c in range(nc)] + [B - 2], np.int64)
    w = np.asarray(words, np.uint32).astype(np.int64)
    c, q = w & 0xFFFF, (w >> 24) & 31
    ci = np.minimum(c, nc - 1)
    ok = (c < nc) & ((w & L.ODPG_OUT_CLS_DROP) == 0) & (q < qb[ci + 1] - qb[ci])
    b = np.where(ok, qb[ci] + q, np.where(c == L.ODPG_COS_NOCLS, B - 2, B - 1))
    return (b, np.argsort(b, kind="stable").astype(np.uint32),
            np.concatenate([[0], np.cumsum(np.bincount(b, minlength=B))]).astype(np.uint32))


def test_deliver_abi_declared():
    """Header, exports and bindings of the new entry points (no GPU)."""
    for f in ("create", "destroy", "num_buckets", "queue_base", "match"):
        assert hasattr(L.lib, "odpg_deliver_" + f) and "odpg_deliver_" + f in L.SIGNATURES
    assert L.SIGNATURES["odpg_deliver"][1] == [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p,
                                               C.c_void_p]
    assert T == 4096 and L.deliver_pktin(10) == 8 and L.deliver_free(10) == 9
    # null handles are refused before any device call
    assert L.lib.odpg_deliver_create(None, None, 1, None) == -22
    assert L.lib.odpg_deliver(None, None, 0, None, None) == -22
    assert L.lib.odpg_deliver_num_buckets(None) == 0
    assert L.lib.odpg_deliver_queue_base(None, 0) < 0 and L.lib.odpg_deliver_match(None, None) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("kind,num,hostile", [
    *[("mixed", n, False) for n in (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)],
    ("mixed", T + 1, True), ("wide", 2 * T + 3, False), ("c4", 2 * T + 3, False)])
def test_random_words(gpu_ctx, fresh_cls, kind, num, hostile):
    """CoS, hash queue, flag bits and sentinels drawn at random. hostile: a
    share of words with a CoS >= num_cos below the sentinels or a hash queue
    >= nq[c]; they land in ODPG_DELIVER_FREE."""
    _, plan, _ = make_plan(fresh_cls, gpu_ctx, kind, num)
    nc, B = plan.num_cos, plan.num_buckets
    assert B == {"mixed": sum(MIXED) + 2, "wide": 2563, "c4": 1027}[kind]
    nq = np.diff([plan.queue_base(c) for c in range(nc)] + [B - 2])
    rng = np.random.default_rng(1000 + num)
    c = rng.integers(0, nc, num)
    w = c | (rng.integers(0, 32, num) % nq[c]) << 24 | rng.integers(0, 16, num) << 16
    if kind == "mixed":
        w[c == nc - 1] |= L.ODPG_OUT_CLS_DROP
    s = rng.random(num) < 0.15
    w[s] = rng.choice(SENTINELS, num)[s] | L.ODPG_OUT_PARSE_ERR
    if hostile:
        h = rng.random(num) < 0.3
        w[h] = (rng.integers(nc, 0xFFFC, num) | rng.integers(0, 32, num) << 24)[h]
        h = rng.random(num) < 0.3
        w[h] = (c | np.minimum(nq[c] + rng.integers(0, 8, num), 31) << 24)[h]
    b, order_ref, offsets_ref = expected(plan, w)
    if num > T and kind != "mixed":
        assert len(np.unique(b & 63)) > 8 and len(np.unique(b >> 6)) > 8
    order, offsets = plan.run(w.astype(np.uint32))
    assert offsets[B] == num and np.array_equal(offsets, offsets_ref)
    assert np.array_equal(order, order_ref)
    if hostile:
        assert offsets[B] - offsets[B - 1] > num // 4


@pytest.mark.gpu
@pytest.mark.parametrize("pattern", ["one_bucket", "sentinels", "alternate"])
def test_skew(gpu_ctx, fresh_cls, pattern):
    """A whole batch in one delivered bucket (the narrow wave counters at
    their largest), only sentinels, and two buckets alternating (runs of 1)."""
    num = 2 * T + 5
    _, plan, _ = make_plan(fresh_cls, gpu_ctx, "mixed", num)
    i = np.arange(num)
    w = {"one_bucket": np.full(num, 3 | 17 << 24),
         "sentinels": np.array(SENTINELS)[i % 4],
         "alternate": np.where(i & 1, 1 | 6 << 24, 3 | 31 << 24)}[pattern].astype(np.uint32)
    b, order_ref, offsets_ref = expected(plan, w)
    assert len(np.unique(b)) == {"one_bucket": 1, "sentinels": 2, "alternate": 2}[pattern]
    order, offsets = plan.run(w)
    assert np.array_equal(offsets, offsets_ref) and np.array_equal(order, order_ref)


@pytest.mark.gpu
def test_after_classify(gpu_ctx, fresh_cls):
    """classify and deliver back to back on the context stream, no sync in
    between: lists of the oracle's verdicts; bucket sizes = the delivered
    counts a counted launch of the same batch folds."""
    num = 3 * T + 17
    tbl, plan, rules = make_plan(fresh_cls, gpu_ctx, "c2", num)
    B = plan.num_buckets
    frames = gen.c2_frames(num, seed=77)
    o = oracle.classify(rules, frames, num, stride=64, opt=ALL_CHKSUM)
    cnt = gpu_ctx.counters(tbl)
    fb, ob = gpu_ctx.buffer(frames.nbytes + 64), gpu_ctx.buffer(4 * num)
    rb, sb = gpu_ctx.buffer(4 * num), gpu_ctx.buffer(4 * (B + 1))
    fb.upload(frames)
    gpu_ctx.classify_dev(tbl, fb, num, stride=64, opt=ALL_CHKSUM, out_buf=ob, counters=cnt)
    plan.run_dev(ob, num, rb, sb)
    gpu_ctx.sync()
    order, offsets = rb.download(np.uint32, num), sb.download(np.uint32, B + 1)
    _, order_ref, offsets_ref = expected(plan, o["out"])
    assert np.array_equal(offsets, offsets_ref) and np.array_equal(order, order_ref)
    queue = cnt.fold()["queue"]
    assert np.array_equal(queue, expected_counters(o, tbl.num_cos)["queue"])
    for c in range(tbl.num_cos):
        qb = plan.queue_base(c)
        assert np.array_equal(np.diff(offsets[qb:qb + 2]), queue[c, :1])
    assert not np.any(queue[:, 1:]) and offsets[B - 2] == queue.sum()


@pytest.mark.gpu
def test_arguments(gpu_ctx, fresh_cls):
    """-EINVAL without a launch for num > max_pkts and null pointers;
    num == 0 zeroes offsets; match() follows the queue layout."""
    tbl, plan, _ = make_plan(fresh_cls, gpu_ctx, "mixed", 100)
    B = plan.num_buckets
    ob, rb, sb = gpu_ctx.buffer(400), gpu_ctx.buffer(400), gpu_ctx.buffer(4 * (B + 1))
    sb.upload(np.full(B + 1, 0xABCD, np.uint32))
    for args in ((ob.ptr, 101, rb.ptr, sb.ptr), (None, 10, rb.ptr, sb.ptr),
                 (ob.ptr, 10, None, sb.ptr), (ob.ptr, 10, rb.ptr, None)):
        assert L.lib.odpg_deliver(plan.h, *args) == -22
    gpu_ctx.sync()
    assert np.all(sb.download(np.uint32, B + 1) == 0xABCD)
    plan.run_dev(ob, 0, rb, sb)
    gpu_ctx.sync()
    assert not np.any(sb.download(np.uint32, B + 1))
    assert L.lib.odpg_deliver_match(plan.h, tbl.h) == 1
    assert L.lib.odpg_deliver_queue_base(plan.h, plan.num_cos) < 0
    fresh_cls.reset()
    other, _, _ = make_plan(fresh_cls, gpu_ctx, "c2", 1)
    assert L.lib.odpg_deliver_match(plan.h, other.h) == 0
