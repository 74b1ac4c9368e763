"""Counted launches on both launch lanes (include/odpg.h "Launch lanes" and
"sharded counters", odp_amd/csrc/lanes.h): a counters object holds a set of
rows per lane, odpg_classify launches that add into it alternate between the
two streams like verdict-only ones, and nothing a caller can observe changes.
Every case checks verdict words bit-exact against the CPU oracle and the
folds against helpers.expected_counters; odpg_counters_fold_lane (a test
entry, odpg_internal.h) shows which lane's rows a launch added into. Sizes as
in test_lanes.py: 4096 + 37 (a partial last tile, several workgroups), 2^18
where one launch has to outlast the next one's start, 64 frames for the
launch that would finish first."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle
import rulesets
from helpers import ALL_CHKSUM, assert_counters, expected_counters, pack
from odp_amd import _lib as L
from odp_amd import cls, gen, gpu

lib = L.lib
N1 = 4096 + 37
BIG = 1 << 18
EINVAL = -22

lib.odpg_counters_fold_lane.restype = C.c_int
lib.odpg_counters_fold_lane.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]

# (frames, seed) of the references, per C2 table (with / without CoS counters)
CASES = {True: [(BIG, 7), (BIG, 9), (64, 8)] + [(N1, 100 + k) for k in range(4)],
         False: [(BIG, 7), (BIG, 9), (N1, 100)]}


class Refs:
    """The C2 table images (with CoS counters: the general kernel counts;
    without: the lean 64-byte kernel does) and, per (stats, n, seed), the
    frames, the oracle's verdicts and the counters they imply: computed once,
    shared by every case and left unchanged."""

    def __init__(self):
        self.image, self.ncos, self.ref = {}, {}, {}
        for stats, cases in CASES.items():
            cls.reset()
            p = cls.loop_pktio(pktin=ALL_CHKSUM)
            gen.build_c2_rules(cls, p, stats=stats)
            assert cls.pktio_start(p) == 0
            rules = cls.pktio_rules(p)
            self.image[stats] = gpu.compile_rules(rules)
            self.ncos[stats] = int(rules.num_cos)
            for n, seed in cases:
                f = gen.c2_frames(n, seed=seed)
                o = oracle.classify(rules, f, n, stride=64, opt=ALL_CHKSUM)
                e = expected_counters(o, self.ncos[stats])
                out = np.array(o["out"])
                for a in (f, out, *e.values()):
                    a.setflags(write=False)
                self.ref[(stats, n, seed)] = (f, out, e)
        cls.reset()


@pytest.fixture(scope="module")
def refs():
    return Refs()


def times(e, k):
    return {x: v * np.uint64(k) for x, v in e.items()}


def plus(*es):
    return {x: sum((e[x] for e in es[1:]), es[0][x].copy()) for x in es[0]}


def fold_lane(cnt, lane):
    """odpg_counters_fold_lane as Counters.fold() returns it, or the error."""
    w = np.zeros(cnt.words, np.uint64)
    rc = lib.odpg_counters_fold_lane(cnt.h, lane, w.ctypes.data_as(C.POINTER(C.c_uint64)))
    if rc:
        return rc
    n = cnt.num_cos
    return {"pktio": w[:4], "cos": w[4:4 + n], "queue": w[4 + n:].reshape(n, L.COS_QUEUE_MAX)}


def launch(ctx, tbl, fb, n, ob, cnt, desc=None, stride=64, opt=ALL_CHKSUM):
    ctx.classify_dev(tbl, fb, n, stride, desc, opt, out_buf=ob, counters=cnt)


class Sets:
    """Device (frames, out) sets of a context over the references `keys`."""

    def __init__(self, ctx, refs, keys):
        self.ctx, self.sets = ctx, []
        for key in keys:
            f, out, e = refs.ref[key]
            fb, ob = ctx.buffer(f.nbytes), ctx.buffer(4 * key[1])
            fb.upload(f)
            ob.zero()
            self.sets.append((fb, ob, key[1], out, e))

    def __getitem__(self, k):
        return self.sets[k]

    def __len__(self):
        return len(self.sets)

    def check_outs(self, which=None):
        for k in range(len(self.sets)) if which is None else which:
            fb, ob, n, out, e = self.sets[k]
            assert np.array_equal(ob.download(np.uint32, n), out), f"verdicts of set {k}"

    def free(self):
        for fb, ob, *_ in self.sets:
            fb.free()
            ob.free()


@pytest.fixture
def ctx():
    c = gpu.Context(0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("stats", [True, False])
@pytest.mark.parametrize("nset", [4, 5])
def test_twelve_counted_launches_over_a_ring(ctx, refs, nset, stats):
    """No sync between the launches. Sets alternate between two frame
    captures, so over a ring of 4 (a set is reused on the lane that used it
    last) lane 0 counts one capture six times and lane 1 the other."""
    assert lib.odpg_ctx_lanes(ctx.h) == 2
    tbl = ctx.table(image=refs.image[stats])
    cnt = ctx.counters(tbl)
    s = Sets(ctx, refs, [(stats, BIG, 7 if k % 2 == 0 else 9) for k in range(nset)])
    for k in range(12):
        fb, ob, n, _, _ = s[k % nset]
        launch(ctx, tbl, fb, n, ob, cnt)
    assert lib.odpg_last_kernel() == (0 if stats else 1)
    e7, e9 = refs.ref[(stats, BIG, 7)][2], refs.ref[(stats, BIG, 9)][2]
    if nset == 4:
        assert_counters(fold_lane(cnt, 0), times(e7, 6), "lane 0")
        assert_counters(fold_lane(cnt, 1), times(e9, 6), "lane 1")
        z = cnt.fold()
        assert not any(np.any(z[x]) for x in z), "rows left after both lane folds"
        for k in range(12):
            fb, ob, n, _, _ = s[k % nset]
            launch(ctx, tbl, fb, n, ob, cnt)
        assert_counters(cnt.fold(), plus(times(e7, 6), times(e9, 6)), "12 launches")
    else:
        n7 = sum(1 for k in range(12) if (k % nset) % 2 == 0)
        f0, f1 = fold_lane(cnt, 0), fold_lane(cnt, 1)
        assert f0["pktio"][0] > 0 and f1["pktio"][0] > 0, "a lane counted nothing"
        want = plus(times(e7, n7), times(e9, 12 - n7))
        assert_counters(plus(f0, f1), want, "lane folds")
        # and through the public fold, which sums both sets
        for k in range(12):
            fb, ob, n, _, _ = s[k % nset]
            launch(ctx, tbl, fb, n, ob, cnt)
        assert_counters(cnt.fold(), want, "12 launches")
    s.check_outs()
    cnt.close()
    s.free()
    del tbl


@pytest.mark.gpu
def test_short_launch_finishes_first(ctx, refs):
    tbl = ctx.table(image=refs.image[True])
    cnt = ctx.counters(tbl)
    s = Sets(ctx, refs, [(True, BIG, 7), (True, 64, 8)])
    for fb, ob, n, _, _ in s:
        launch(ctx, tbl, fb, n, ob, cnt)
    assert_counters(cnt.fold(), plus(s[0][4], s[1][4]), "long + short")
    s.check_outs()
    cnt.close()
    s.free()
    del tbl


@pytest.mark.gpu
def test_counted_and_verdict_only_across_a_fold(ctx, refs):
    tbl = ctx.table(image=refs.image[True])
    cnt = ctx.counters(tbl)
    s = Sets(ctx, refs, [(True, N1, 100 + k) for k in range(4)])
    want = None
    for half, kinds in enumerate(("CVCCVC", "VCCVCC")):
        counted = []
        for k, kind in enumerate(kinds):
            fb, ob, n, _, e = s[(k + half) % 4]
            launch(ctx, tbl, fb, n, ob, cnt if kind == "C" else None)
            if kind == "C":
                counted.append(e)
        want = plus(*counted)
        assert_counters(cnt.fold(), want, f"fold {half}")
    z = cnt.fold()
    assert not any(np.any(z[x]) for x in z)
    s.check_outs()
    cnt.close()
    s.free()
    del tbl


class Part(gpu.DeviceBuffer):
    """A range of a device buffer, with the buffer's upload / zero / download."""

    def __init__(self, whole, off, nbytes):
        self.ctx, self.ptr, self.nbytes = whole.ctx, whole.ptr + off, int(nbytes)

    def free(self):
        self.ptr = None


def alternating_case(ctx, tbl, frames, n, e, out, kernel, desc=None, stride=64, opt=ALL_CHKSUM):
    """Four counted launches of one batch into four outs that conflict
    nowhere, so they alternate and each lane's rows hold exactly two
    launches' counts. A descriptor batch may read anywhere in the 8 GiB above
    its frames (the span its descriptor format addresses, odpg_classify), and
    an out in there would keep its launch on the lane of the one before. So
    every buffer is a part of one allocation, the outs first, then the
    descriptors, the frames last: no launch writes what another may read,
    wherever the allocation lies."""
    _, desc_dt = L.np_dtypes()
    if desc is not None:
        desc = np.ascontiguousarray(desc, dtype=desc_dt)
    up = lambda x: (int(x) + 255) & ~255
    osz, dsz = up(4 * n), up(desc.nbytes) if desc is not None else 0
    whole = ctx.buffer(4 * osz + dsz + frames.nbytes + 256)
    obs = [Part(whole, k * osz, 4 * n) for k in range(4)]
    db = Part(whole, 4 * osz, desc.nbytes) if desc is not None else None
    fb = Part(whole, 4 * osz + dsz, frames.nbytes + 256)
    assert all(ob.ptr + ob.nbytes <= (db or fb).ptr for ob in obs) and \
        (db is None or db.ptr + db.nbytes <= fb.ptr)
    whole.zero()
    fb.upload(frames)
    if db:
        db.upload(desc)
    cnt = ctx.counters(tbl)
    for ob in obs:
        launch(ctx, tbl, fb, n, ob, cnt, db, stride, opt)
    assert lib.odpg_last_kernel() == kernel
    assert e["pktio"][0] > 0            # so 2 x e on lane 1 proves lane 1 counted
    for lane in (0, 1):
        f = fold_lane(cnt, lane)
        assert_counters(f, times(e, 2), f"lane {lane}")
    for k, ob in enumerate(obs):
        assert np.array_equal(ob.download(np.uint32, n), out), f"launch {k}"
    cnt.close()
    whole.free()


@pytest.mark.gpu
def test_cos_keyed_lean_kernel(ctx, fresh_cls):
    """C4 (1024 PMRs, raised limits): the lean kernel's CoS-keyed
    instantiation, whose counters leave through the barrier flush."""
    assert fresh_cls.set_limits(2048, 2048, 32) == 0
    p = fresh_cls.loop_pktio(pktin=ALL_CHKSUM)
    gen.build_c4_rules(fresh_cls, p)
    assert fresh_cls.pktio_start(p) == 0
    rules = fresh_cls.pktio_rules(p)
    fr = gen.c2_frames(N1, seed=41)
    o = oracle.classify(rules, fr, N1, stride=64, opt=ALL_CHKSUM)
    tbl = ctx.table(rules)
    alternating_case(ctx, tbl, fr, N1, expected_counters(o, tbl.num_cos), o["out"], 1)
    del tbl


@pytest.mark.gpu
def test_descriptor_kernel(ctx, fresh_cls):
    p = fresh_cls.loop_pktio(pktin=ALL_CHKSUM)
    gen.build_c3_rules(fresh_cls, p)
    assert fresh_cls.pktio_start(p) == 0
    rules = fresh_cls.pktio_rules(p)
    buf, desc = gen.c3_frames(N1, seed=42)
    o = oracle.classify(rules, buf, N1, desc=desc, opt=ALL_CHKSUM)
    tbl = ctx.table(rules)
    alternating_case(ctx, tbl, buf, N1, expected_counters(o, tbl.num_cos), o["out"], 2,
                     desc=desc, stride=0)
    del tbl


@pytest.mark.gpu
def test_general_kernel_forced(ctx, refs):
    """The C2 table the lean kernel would take, under a forced strategy."""
    f, out, e = refs.ref[(False, N1, 100)]
    tbl = ctx.table(image=refs.image[False])
    ctx.set_kernel_mode(2)
    alternating_case(ctx, tbl, f, N1, e, out, 0)
    del tbl


@pytest.mark.gpu
def test_hash_queue_columns(ctx, fresh_cls):
    """num_queue > 1 CoS: the non-identity queue column path."""
    p = fresh_cls.loop_pktio()
    d = fresh_cls.cos_create("d", num_queue=7, stats_enable=True,
                             hash_proto=fresh_cls.HASH_IPV4 | fresh_cls.HASH_IPV4_UDP)
    x = fresh_cls.cos_create("x", queue=fresh_cls.queue(3), num_queue=1)
    y = fresh_cls.cos_create("y", num_queue=3, hash_proto=fresh_cls.HASH_IPV4,
                             stats_enable=True)
    fresh_cls.default_cos_set(p, d)
    assert fresh_cls.pmr_create([fresh_cls.Term(fresh_cls.PMR_IPPROTO, b"\x06", b"\xff")], d, x)
    assert fresh_cls.pmr_create([fresh_cls.Term(fresh_cls.PMR_UDP_DPORT, b"\x00\x07",
                                                b"\x00\x07")], d, y)
    assert fresh_cls.pktio_start(p) == 0
    frames = rulesets.mutate_corpus(N1, seed=5)
    buf, desc = pack(frames)
    rules = fresh_cls.pktio_rules(p)
    o = oracle.classify(rules, buf, N1, desc=desc)
    tbl = ctx.table(rules)
    e = expected_counters(o, tbl.num_cos)
    assert np.count_nonzero(e["queue"][fresh_cls.to_index(d)]) > 1
    alternating_case(ctx, tbl, buf, N1, e, o["out"], 0, desc=desc, stride=0, opt=0)
    del tbl


def _hip():
    """The HIP runtime libodpg.so brought into the process."""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["set_lanes", "caller_stream"])
def test_one_lane_contexts(how, refs):
    stream = None
    if how == "caller_stream":
        hip = _hip()
        stream = C.c_void_p()
        assert hip.hipSetDevice(0) == 0
        assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0     # non-blocking
    c = gpu.Context(0, stream)
    try:
        if how == "set_lanes":
            assert lib.odpg_ctx_set_lanes(c.h, 1) == 0
        assert lib.odpg_ctx_lanes(c.h) == 1
        tbl = c.table(image=refs.image[True])
        cnt = c.counters(tbl)
        s = Sets(c, refs, [(True, N1, 100 + k) for k in range(4)])
        for fb, ob, n, _, _ in s:
            launch(c, tbl, fb, n, ob, cnt)
        f1 = fold_lane(cnt, 1)
        if how == "caller_stream":
            assert f1 == EINVAL
        else:
            assert not any(np.any(f1[x]) for x in f1), "lane 1 counted on a one-lane context"
        total = plus(*(x[4] for x in s))
        assert_counters(cnt.fold(), total, "one lane")
        if how == "set_lanes":
            # 1 -> 2 -> 1 between launches, one fold at the end
            for lanes in (1, 2, 2, 1, 1, 2):
                assert lib.odpg_ctx_set_lanes(c.h, lanes) == 0
                for fb, ob, n, _, _ in s:
                    launch(c, tbl, fb, n, ob, cnt)
            assert_counters(cnt.fold(), times(total, 6), "lanes switched between launches")
        s.check_outs()
        cnt.close()
        s.free()
        del tbl
    finally:
        c.close()
        if stream is not None:
            hip.hipStreamDestroy(stream)


@pytest.mark.gpu
def test_destroy_behind_launches_on_both_lanes(ctx, refs):
    """odpg_counters_destroy with launches in flight on both lanes returns
    and nothing crashes; the launches' verdicts are exact afterwards. (A
    destroy that did not wait for lane 1 would free rows still written to,
    which verdict words cannot show: this case does not prove the wait.)"""
    tbl = ctx.table(image=refs.image[True])
    cnt = ctx.counters(tbl)
    s = Sets(ctx, refs, [(True, BIG, 7), (True, BIG, 9)])
    for fb, ob, n, _, _ in s:
        launch(ctx, tbl, fb, n, ob, cnt)
    cnt.close()
    s.check_outs()
    s.free()
    del tbl


@pytest.mark.gpu
def test_recv_batches_without_sync(gpu_ctx, fresh_cls):
    """odpg_pktio_recv_batch with device pointers passes the binding's
    counters: eight calls over four buffer sets, then the statistics."""
    p = fresh_cls.loop_pktio(pktin=ALL_CHKSUM)
    r = gen.build_c2_rules(fresh_cls, p, stats=True)
    assert fresh_cls.pktio_start(p) == 0
    n = N1
    fr = gen.c2_frames(n, seed=9)
    o = oracle.classify(fresh_cls.pktio_rules(p), fr, n, stride=64, opt=ALL_CHKSUM)
    fbs, obs = [], []
    for _ in range(4):
        fbs.append(gpu_ctx.buffer(fr.nbytes))
        fbs[-1].upload(fr)
        obs.append(gpu_ctx.buffer(4 * n))
        obs[-1].zero()
    for k in range(8):
        assert lib.odpg_pktio_recv_batch(p, gpu_ctx.h, fbs[k % 4].ptr, None, 64, n, 1,
                                         obs[k % 4].ptr, None) == 0
    st = fresh_cls.pktio_stats(p)
    got = [st.in_packets, st.in_octets, st.in_errors, st.in_discards]
    assert got == [8 * int(x) for x in o["stats"][:4]]
    for leaf in r["leaves"]:
        i = fresh_cls.to_index(leaf)
        rc, cs = fresh_cls.cos_stats(leaf)
        assert rc == 0 and cs.packets == 8 * int(o["stats"][4 + i]), i
        rc, qs = fresh_cls.queue_stats(leaf, fresh_cls.cos_queue(leaf))
        assert rc == 0 and qs.packets == 8 * int(((o["out"] & 0xFFFF) == i).sum()), i
    for k, ob in enumerate(obs):
        assert np.array_equal(ob.download(np.uint32, n), o["out"]), f"set {k}"
    for b in fbs + obs:
        b.free()


def test_fold_lane_entry_point():
    """Exported, not public API, and null handles refused before any device call (no GPU)."""
    assert "odpg_counters_fold_lane" not in L.SIGNATURES
    w = (C.c_uint64 * 8)()
    assert lib.odpg_counters_fold_lane(None, 0, w) == EINVAL


def test_join_bookkeeping_against_model():
    """odp_amd/csrc/lanes.h (plain C) driven by tests/c/lanes_join_model.cpp,
    built with AddressSanitizer + UBSan and run as a plain executable: launch /
    join call patterns on vector clocks."""
    cdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c")
    r = subprocess.run(["make", "-s", "-C", cdir, "-f", "lanes_join_model.mk"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(cdir, "lanes_join_model.asan")], capture_output=True,
                       text=True, timeout=300)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "PASS: joins" in r.stdout, out[-4000:]
    for what in ("(a) disjoint buffers: 1000 iterations, 0 events",
                 "(a) one buffer set: 1000 iterations, 0 events",
                 "(b) disjoint buffers: 1000", "(b) two buffer sets: 1000", "(c) lane_set"):
        assert what in r.stdout, out[-4000:]
