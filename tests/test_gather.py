"""Dense per-queue frame batches (include/odpg_gather.h).

odpg_gather() writes the frames of a range of delivery buckets back to back
in delivery order. Reference: numpy on the same inputs (a fancy index for a
fixed stride, a cumulative sum of align16(len) and a plain loop for
descriptors); bytes and integers, compared exactly. Every destination buffer
is prefilled with 0xA5, so a write outside the gathered region shows.
T = the tile of positions one workgroup handles."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import ALL_CHKSUM
from odp_amd import _lib as L
from odp_amd import gen
from test_deliver import expected as deliver_lists

T = L.GATHER_TILE
SIZES = (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)
LENS = (0, 1, 15, 16, 17, 60, 64, 65, 570, 1518)
DESC_DT = L.np_dtypes()[1]
TOTAL_DT = np.dtype(L.GATHER_TOTAL_FIELDS)
# 6 buckets (bucket 2 is empty): all of them, a middle range, two empty ranges
RANGES = ((0, 6), (1, 4), (3, 3), (2, 3))


def expected(frames, order, offsets, b_first, b_last, cap, stride=0, desc=None, words=None):
    """(frames[cap + 64], desc[num], words[num] or None, total) of the header's rules."""
    num = len(order)
    e = min(int(offsets[b_last]), num)
    s = min(int(offsets[b_first]), e)
    idx = order[s:e].astype(np.int64)
    ok = idx < num
    i = np.where(ok, idx, 0)
    ln = np.where(ok, desc["len"][i], 0).astype(np.int64) if desc is not None \
        else np.full(e - s, stride, np.int64)
    src = desc["offset"][i].astype(np.int64) if desc is not None else i * stride
    al = (ln + 15) // 16 * 16
    off = np.cumsum(al) - al
    copied = int(np.count_nonzero(off + al <= cap))
    out = np.full(cap + 64, 0xA5, np.uint8)
    d = np.full(num, 0xA5A5A5A5, np.uint32).repeat(2).view(DESC_DT)
    d[:e - s] = (0, 0)
    d["offset"][:copied], d["len"][:copied] = off[:copied], ln[:copied]
    for j in range(copied):
        out[off[j]:off[j] + al[j]] = 0
        if ok[j]:
            out[off[j]:off[j] + ln[j]] = frames[src[j]:src[j] + ln[j]]
    w = None
    if words is not None:
        w = np.full(num, 0xA5A5A5A5, np.uint32)
        w[:e - s] = np.where(ok, words[i], 0)
    return out, d, w, np.array((e - s, copied, al.sum()), TOTAL_DT)


def run_and_check(plan, frames, order, offsets, b_first, b_last, cap=None, **src):
    """Gather on the GPU, compare every output with expected(); returns the reference."""
    if cap is None:
        cap = len(order) * src["stride"] if src.get("desc") is None else \
            int(((src["desc"]["len"].astype(np.int64) + 15) // 16 * 16).sum())
    got = plan.run(frames, order, offsets, b_first, b_last, capacity=cap, fill=0xA5, **src)
    ref = expected(frames, order, offsets, b_first, b_last, cap, **src)
    for name, g, r in zip(("frames", "desc", "words", "total"), got, ref):
        assert np.asarray(g).tobytes() == np.asarray(r).tobytes(), (name, g, r)
    assert np.all(got[0][min(int(ref[3]["bytes"]), cap):] == 0xA5)
    return ref


def make_batch(rng, num, lens=None):
    """order / offsets of RANGES' 6 buckets, words, and either fixed-stride bytes
    (lens None) or descriptors whose frames lie shuffled in the buffer."""
    cuts = np.sort(rng.integers(0, num + 1, 4))
    offsets = np.array([0, cuts[0], cuts[1], cuts[1], cuts[2], cuts[3], num], np.uint32)
    order, words = rng.permutation(num).astype(np.uint32), rng.integers(0, 1 << 32, num, np.uint32)
    if lens is None:
        return order, offsets, words, None
    al, place = (lens + 15) // 16 * 16, rng.permutation(num)
    desc = np.zeros(num, DESC_DT)
    desc["len"] = lens
    desc["offset"][place] = np.cumsum(al[place]) - al[place]
    return order, offsets, words, desc


def test_gather_abi_declared():
    """Header, exports and bindings of the new entry points (no GPU)."""
    for f in ("odpg_gather_create", "odpg_gather_destroy", "odpg_gather"):
        assert hasattr(L.lib, f) and f in L.SIGNATURES
    assert T == 1024 and TOTAL_DT.itemsize == C.sizeof(L.odpg_gather_total_t) == 16
    assert C.sizeof(L.odpg_gather_src_t) == 32 and C.sizeof(L.odpg_gather_dst_t) == 40
    # null handles are refused before any device call
    assert L.lib.odpg_gather_create(None, 1, None) == -22
    assert L.lib.odpg_gather(None, None, None, None, 0, 0, None) == -22
    L.lib.odpg_gather_destroy(None)


@pytest.mark.gpu
@pytest.mark.parametrize("num", SIZES)
@pytest.mark.parametrize("stride", [16, 64, 80])
def test_fixed_stride(gpu_ctx, stride, num):
    rng = np.random.default_rng(2000 + num + stride)
    order, offsets, words, _ = make_batch(rng, num)
    frames = rng.integers(0, 256, num * stride, np.uint8)
    plan = gpu_ctx.gather(num)
    for bf, bl in RANGES:
        run_and_check(plan, frames, order, offsets, bf, bl, stride=stride, words=words)
    run_and_check(plan, frames, order, offsets, 0, 6, stride=stride)   # without words
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("num,lens", [*[(n, LENS) for n in SIZES],
                                      (2 * T + 5, (1518,)), (2 * T + 5, (0,))])
def test_variable_length(gpu_ctx, num, lens):
    rng = np.random.default_rng(3000 + num + len(lens))
    order, offsets, words, desc = make_batch(rng, num, rng.choice(lens, num))
    frames = rng.integers(0, 256, int(desc["offset"].max()) + 1518 + 64, np.uint8)
    plan = gpu_ctx.gather(num)
    for bf, bl in RANGES:
        run_and_check(plan, frames, order, offsets, bf, bl, desc=desc, words=words)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["middle", "zero"])
def test_capacity(gpu_ctx, where):
    """Capacity inside the middle frame: the frames before it are copied, the
    rest has desc {0, 0}, total.bytes is the full need."""
    num = T + 1
    rng = np.random.default_rng(4000)
    lens = rng.choice(LENS, num)
    order = rng.permutation(num).astype(np.uint32)
    lens[order[num // 2]] = 570
    _, _, words, desc = make_batch(rng, num, lens)
    offsets = np.array([0, num], np.uint32)
    frames = rng.integers(0, 256, int(desc["offset"].max()) + 1518 + 64, np.uint8)
    al = (lens[order].astype(np.int64) + 15) // 16 * 16
    cap = int(al[:num // 2].sum()) + 285 if where == "middle" else 0
    plan = gpu_ctx.gather(num)
    ref = run_and_check(plan, frames, order, offsets, 0, 1, cap, desc=desc, words=words)
    if where == "middle":
        assert ref[3]["copied"] == num // 2
    assert ref[3]["bytes"] == al.sum() > cap and ref[3]["num"] == num
    run_and_check(plan, frames, order, offsets, 0, 1, 64 * (num // 2) + 63, stride=64)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hostile", ["order", "last", "first"])
def test_hostile_lists(gpu_ctx, hostile):
    """order entries >= num, offsets[b_last] > num, offsets[b_first] >
    offsets[b_last]: clamped as the header says, canaries intact."""
    num = T + 1
    rng = np.random.default_rng(5000)
    order, offsets, words, desc = make_batch(rng, num, rng.choice(LENS, num))
    frames = rng.integers(0, 256, int(desc["offset"].max()) + 1518 + 64, np.uint8)
    bf, bl = 0, 6
    if hostile == "order":
        bad = rng.random(num) < 0.2
        order[bad] = rng.choice([num, num + 1, 1 << 31, 0xFFFFFFFF], num)[bad]
    elif hostile == "last":
        offsets[6] = num + 5000
    else:
        offsets[1], bf, bl = offsets[4] + 7, 1, 4
    plan = gpu_ctx.gather(num)
    ref = run_and_check(plan, frames, order, offsets, bf, bl, desc=desc, words=words)
    assert ref[3]["num"] == (0 if hostile == "first" else num)
    run_and_check(plan, frames[:64 * num], order, offsets, bf, bl, stride=64, words=words)
    plan.close()


@pytest.mark.gpu
@pytest.mark.parametrize("config", ["c3", "c2"])
def test_chain_without_sync(gpu_ctx, fresh_cls, config):
    """classify -> deliver -> gather of the delivered buckets -> classify of
    the gathered batch, one sync at the end: the dense batch is a valid batch
    for the existing kernels and its verdicts are the first pass's, in
    delivery order."""
    num = 3 * T + 17
    p = fresh_cls.loop_pktio(pktin=ALL_CHKSUM)
    (gen.build_c3_rules if config == "c3" else gen.build_c2_rules)(fresh_cls, p)
    assert fresh_cls.pktio_start(p) == 0
    rules = fresh_cls.pktio_rules(p)
    tbl = gpu_ctx.table(rules)
    dplan, gplan = gpu_ctx.deliver(tbl, num), gpu_ctx.gather(num)
    B = dplan.num_buckets
    if config == "c3":
        (frames, desc), stride = gen.c3_frames(num, seed=78), 0
    else:
        frames, desc, stride = gen.c2_frames(num, seed=78), None, 64
    o = oracle.classify(rules, frames, num, stride=stride, desc=desc, opt=ALL_CHKSUM)
    _, order_ref, offsets_ref = deliver_lists(dplan, o["out"])
    n2 = int(offsets_ref[B - 2])
    assert n2 > 2 * T
    bufs = [gpu_ctx.buffer(n) for n in (frames.nbytes + 64, 8 * num, 4 * num, 4 * num,
                                        4 * (B + 1), frames.nbytes + 64, 8 * num, 4 * num, 16,
                                        4 * num)]
    fb, db, ob, rb, sb, gfb, gdb, gwb, tb, ob2 = bufs
    fb.upload(frames)
    if desc is not None:
        db.upload(desc)
    sdesc, ddesc = (db, gdb) if desc is not None else (None, None)
    gpu_ctx.classify_dev(tbl, fb, num, stride=stride, desc_buf=sdesc, opt=ALL_CHKSUM, out_buf=ob)
    dplan.run_dev(ob, num, rb, sb)
    gplan.run_dev(fb, num, rb, sb, 0, B - 2, gfb, frames.nbytes, tb, stride, sdesc, ob, gdb, gwb)
    gpu_ctx.classify_dev(tbl, gfb, n2, stride=stride, desc_buf=ddesc, opt=ALL_CHKSUM, out_buf=ob2)
    gpu_ctx.sync()
    total = tb.download(TOTAL_DT, 1)[0]
    assert total["num"] == total["copied"] == n2
    gwords = gwb.download(np.uint32, n2)
    assert np.array_equal(gwords, o["out"][order_ref[:n2]])
    assert np.array_equal(ob2.download(np.uint32, n2), gwords)
    for b in bufs:
        b.free()
    dplan.close()
    gplan.close()


@pytest.mark.gpu
def test_arguments(gpu_ctx):
    """Every -EINVAL case of the header returns before a launch: a
    canary-filled total is unchanged after a sync."""
    plan = gpu_ctx.gather(100)
    fb, db, wb, rb, sb, tb = (gpu_ctx.buffer(6400) for _ in range(6))
    tb.upload(np.full(4, 0xABCD, np.uint32))
    good_s = dict(frames=fb.ptr, desc=db.ptr, stride=0, num=100, words=wb.ptr)
    good_d = dict(frames=fb.ptr, capacity=6400, desc=db.ptr, words=wb.ptr, total=tb.ptr)
    cases = [({}, {}, dict(g=None)), ({}, {}, dict(order=None)), ({}, {}, dict(offsets=None)),
             ({}, {}, dict(src=None)), ({}, {}, dict(dst=None)), ({}, {}, dict(b_first=2, b_last=1)),
             ({}, dict(frames=None), {}), ({}, dict(total=None), {}), (dict(num=101), {}, {}),
             ({}, dict(capacity=(1 << 32) + 1), {}), (dict(desc=None, stride=0), {}, {}),
             (dict(desc=None, stride=72), {}, {}), ({}, dict(desc=None), {}),
             ({}, dict(words=None), {}), (dict(words=None), {}, {})]
    for ds, dd, dc in cases:
        s, d = L.odpg_gather_src_t(**{**good_s, **ds}), L.odpg_gather_dst_t(**{**good_d, **dd})
        c = {**dict(g=plan.h, src=C.byref(s), order=rb.ptr, offsets=sb.ptr, b_first=0, b_last=1,
                    dst=C.byref(d)), **dc}
        assert L.lib.odpg_gather(c["g"], c["src"], c["order"], c["offsets"], c["b_first"],
                                 c["b_last"], c["dst"]) == -22, (ds, dd, dc)
    gpu_ctx.sync()
    assert np.all(tb.download(np.uint32, 4) == 0xABCD)
    plan.close()
