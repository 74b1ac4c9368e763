"""Launch lanes (include/odpg.h "Launch lanes", odp_amd/csrc/lanes.h):
verdict-only odpg_classify launches of a context alternate between two
streams, and nothing a caller can observe changes. Every case uses the C2
rules and checks verdict words bit-exact against the CPU oracle:
launches without a sync between them, write-after-write and shared-read
pairs, joins at a read-back, a fence, an event, odpg_deliver and counted
launches, the contexts that keep to one lane, and more launches in flight
than a lane's ring records. Sizes: 4096 + 37 (a partial last tile, several
workgroups), 2^18 where one launch has to outlast the next one's start, and
64 / 320 frames for the short launches that would finish first."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import ALL_CHKSUM, assert_counters, expected_counters
from odp_amd import _lib as L
from odp_amd import cls, gen, gpu

lib = L.lib
N1 = 4096 + 37
BIG = 1 << 18

# (frames, seed) of every reference the cases use, and with CoS counters
CASES = [(N1, 100 + k) for k in range(6)] + [(BIG, 7), (64, 8), (BIG, 9), (7 * 64 * 5, 77)]
CASES_STATS = [(8192 + 5, 55)]


class Refs:
    """The C2 table images (without / with CoS counters) and, per (n, seed),
    the frames and the oracle's result: computed once, while the rule
    snapshot is alive, shared by every case and left unchanged."""

    def __init__(self):
        self.image, self.ref = {}, {}
        for stats, cases in ((False, CASES), (True, CASES_STATS)):
            cls.reset()
            p = cls.loop_pktio(pktin=ALL_CHKSUM)
            gen.build_c2_rules(cls, p, stats=stats)
            assert cls.pktio_start(p) == 0
            rules = cls.pktio_rules(p)
            self.image[stats] = gpu.compile_rules(rules)
            for n, seed in cases:
                f = gen.c2_frames(n, seed=seed)
                o = oracle.classify(rules, f, n, stride=64, opt=ALL_CHKSUM)
                o = {k: np.array(v) for k, v in o.items() if isinstance(v, np.ndarray)}
                for a in (f, *o.values()):
                    a.setflags(write=False)
                self.ref[(n, seed)] = (f, o)
        cls.reset()


@pytest.fixture(scope="module")
def refs():
    return Refs()


@pytest.fixture(scope="module")
def env(refs):
    """A context of its own (two lanes), the C2 table on it, the references."""
    ctx = gpu.Context(0)
    ctx.refs = refs
    tbl = ctx.table(image=refs.image[False])
    yield ctx, tbl
    del tbl
    ctx.close()


def launch(ctx, tbl, frames_ptr, n, out_ptr, counters=None):
    b = L.odpg_batch_t(frames_ptr, None, 64, n, ALL_CHKSUM, L.LAYER_ALL, 1)
    r = L.odpg_result_t(out_ptr, None, None, None, counters.h if counters else None)
    assert lib.odpg_classify(ctx.h, tbl.h, C.byref(b), C.byref(r)) == 0


def device_frames(ctx, n, seed):
    f, o = ctx.refs.ref[(n, seed)]
    fb = ctx.buffer(f.nbytes)
    fb.upload(f)
    return fb, o["out"]


def six_launches(ctx, tbl):
    """Six (frames, out) pairs classified back to back, one sync, all exact."""
    pairs = [device_frames(ctx, N1, 100 + k) + (ctx.buffer(4 * N1),) for k in range(6)]
    for fb, _, ob in pairs:
        ob.zero()
    for fb, _, ob in pairs:
        launch(ctx, tbl, fb.ptr, N1, ob.ptr)
    ctx.sync()
    assert lib.odpg_last_kernel() == 1, "lean kernel not taken"
    for k, (fb, exp, ob) in enumerate(pairs):
        assert np.array_equal(ob.download(np.uint32, N1), exp), f"launch {k}"
    for fb, _, ob in pairs:
        fb.free()
        ob.free()


@pytest.mark.gpu
def test_six_launches_without_sync(env):
    ctx, tbl = env
    assert lib.odpg_ctx_lanes(ctx.h) == 2
    six_launches(ctx, tbl)
    assert lib.odpg_ctx_lanes(ctx.h) == 2


@pytest.mark.gpu
def test_write_after_write_and_shared_read(env):
    """B (64 frames) is launched right behind A (2^18) into the same out
    buffer: B would finish first on a lane of its own and be overwritten.
    Two launches reading the same frames into different outs stay legal."""
    ctx, tbl = env
    fa, ea = device_frames(ctx, BIG, 7)
    fb, eb = device_frames(ctx, 64, 8)
    out, out2 = ctx.buffer(4 * BIG), ctx.buffer(4 * BIG)
    out.zero()
    out2.zero()
    launch(ctx, tbl, fa.ptr, BIG, out.ptr)
    launch(ctx, tbl, fb.ptr, 64, out.ptr)
    ctx.sync()
    got = out.download(np.uint32, BIG)
    assert np.array_equal(got[:64], eb), "the later launch's verdicts were overwritten"
    assert np.array_equal(got[64:], ea[64:])
    launch(ctx, tbl, fa.ptr, BIG, out.ptr)
    launch(ctx, tbl, fa.ptr, BIG, out2.ptr)
    ctx.sync()
    assert np.array_equal(out.download(np.uint32, BIG), ea)
    assert np.array_equal(out2.download(np.uint32, BIG), ea)
    for b in (fa, fb, out, out2):
        b.free()


@pytest.mark.gpu
def test_join_on_read_back(env):
    ctx, tbl = env
    fa, ea = device_frames(ctx, BIG, 7)
    fb, eb = device_frames(ctx, BIG, 9)
    oa, ob = ctx.buffer(4 * BIG), ctx.buffer(4 * BIG)
    oa.zero()
    ob.zero()
    launch(ctx, tbl, fa.ptr, BIG, oa.ptr)
    launch(ctx, tbl, fb.ptr, BIG, ob.ptr)
    # odpg_memcpy_d2h, no odpg_ctx_sync
    assert np.array_equal(ob.download(np.uint32, BIG), eb)
    assert np.array_equal(oa.download(np.uint32, BIG), ea)
    for b in (fa, fb, oa, ob):
        b.free()


@pytest.mark.gpu
def test_fence_and_event_cover_both_lanes(env):
    """Outs in pinned, mapped host memory, read directly after the fence."""
    ctx, tbl = env
    fa, ea = device_frames(ctx, N1, 100)
    fb, eb = device_frames(ctx, N1, 101)
    host, dev = [], []
    for _ in range(2):
        hp, dp = C.c_void_p(), C.c_void_p()
        assert lib.odpg_host_alloc_pinned(4 * N1, C.byref(hp)) == 0
        assert lib.odpg_host_device_ptr(hp, C.byref(dp)) == 0
        C.memset(hp.value, 0, 4 * N1)
        host.append(hp.value)
        dev.append(dp.value)
    fence = C.c_void_p()
    assert lib.odpg_fence_create(ctx.h, C.byref(fence)) == 0
    try:
        launch(ctx, tbl, fa.ptr, N1, dev[0])
        launch(ctx, tbl, fb.ptr, N1, dev[1])
        assert lib.odpg_fence_record(ctx.h, fence) == 0
        assert lib.odpg_fence_wait(fence) == 0
        for hp, exp, what in ((host[0], ea, "first"), (host[1], eb, "second")):
            got = np.frombuffer((C.c_uint32 * N1).from_address(hp), np.uint32)
            assert np.array_equal(got, exp), f"{what} launch incomplete behind the fence"
        assert lib.odpg_event_record(ctx.h, 0) == 0
        launch(ctx, tbl, fa.ptr, N1, dev[0])
        launch(ctx, tbl, fb.ptr, N1, dev[1])
        assert lib.odpg_event_record(ctx.h, 1) == 0
        ms = C.c_float(0)
        assert lib.odpg_event_elapsed_ms(ctx.h, 0, 1, C.byref(ms)) == 0
        assert ms.value > 0
        ctx.sync()
    finally:
        lib.odpg_fence_destroy(fence)
        for hp in host:
            lib.odpg_host_free_pinned(hp)
        fa.free()
        fb.free()


@pytest.mark.gpu
def test_deliver_behind_a_launch(env):
    from test_deliver import expected
    ctx, tbl = env
    plan = ctx.deliver(tbl, N1)
    nb = plan.num_buckets
    sets = []
    for seed in (100, 101):
        fb, exp = device_frames(ctx, N1, seed)
        sets.append((fb, exp, ctx.buffer(4 * N1), ctx.buffer(4 * N1), ctx.buffer(4 * (nb + 1))))
    for fb, _, ob, _, _ in sets:
        launch(ctx, tbl, fb.ptr, N1, ob.ptr)
    # the second launch's out first: whichever lane it ran on
    for fb, _, ob, order, offs in reversed(sets):
        plan.run_dev(ob, N1, order, offs)
    ctx.sync()
    for k, (fb, exp, ob, order, offs) in enumerate(sets):
        _, eo, ef = expected(plan, exp)
        assert np.array_equal(order.download(np.uint32, N1), eo), f"order {k}"
        assert np.array_equal(offs.download(np.uint32, nb + 1), ef), f"offsets {k}"
    plan.close()
    for s in sets:
        for b in (s[0],) + s[2:]:
            b.free()


@pytest.mark.gpu
def test_counted_and_verdict_only_interleaved(refs):
    n = 8192 + 5
    ctx = gpu.Context(0)
    ctx.refs = refs
    tbl = ctx.table(image=refs.image[True])
    cnt = ctx.counters(tbl)
    fb, exp = device_frames(ctx, n, 55)
    e = expected_counters(refs.ref[(n, 55)][1], tbl.num_cos)
    outs = [ctx.buffer(4 * n) for _ in range(6)]
    for ob in outs:
        ob.zero()
    for kind, ob in zip("VCVCCV", outs):
        launch(ctx, tbl, fb.ptr, n, ob.ptr, counters=cnt if kind == "C" else None)
    f = cnt.fold()
    assert_counters(f, {k: v * np.uint64(3) for k, v in e.items()}, "three counted launches")
    assert int(f["pktio"][0]) + int(f["pktio"][2]) == 3 * n and f["cos"].sum() > 0
    ctx.sync()
    for k, ob in enumerate(outs):
        assert np.array_equal(ob.download(np.uint32, n), exp), f"launch {k}"
    cnt.close()
    del tbl
    for b in outs + [fb]:
        b.free()
    ctx.close()


def _hip():
    """The HIP runtime libodpg.so brought into the process."""
    for ln in open("/proc/self/maps"):
        if "libamdhip64" in ln:
            return C.CDLL(ln.split()[-1])
    raise RuntimeError("libamdhip64 is not loaded")


@pytest.mark.gpu
@pytest.mark.parametrize("how", ["caller_stream", "stream_handed_out", "set_lanes"])
def test_one_lane_contexts(how, refs):
    stream = None
    if how == "caller_stream":
        hip = _hip()
        stream = C.c_void_p()
        assert hip.hipSetDevice(0) == 0
        assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0     # non-blocking
    ctx = gpu.Context(0, stream)
    ctx.refs = refs
    try:
        if how == "stream_handed_out":
            assert lib.odpg_ctx_lanes(ctx.h) == 2
            assert lib.odpg_ctx_stream(ctx.h)
        elif how == "set_lanes":
            assert lib.odpg_ctx_lanes(ctx.h) == 2
            assert lib.odpg_ctx_set_lanes(ctx.h, 1) == 0
        assert lib.odpg_ctx_lanes(ctx.h) == 1
        if how != "set_lanes":
            assert lib.odpg_ctx_set_lanes(ctx.h, 2) < 0
        tbl = ctx.table(image=refs.image[False])
        six_launches(ctx, tbl)
        assert lib.odpg_ctx_lanes(ctx.h) == 1
        if how == "set_lanes":      # and on again
            assert lib.odpg_ctx_set_lanes(ctx.h, 2) == 0 and lib.odpg_ctx_lanes(ctx.h) == 2
            six_launches(ctx, tbl)
        del tbl
    finally:
        ctx.close()
        if stream is not None:
            hip.hipStreamDestroy(stream)


@pytest.mark.gpu
def test_more_launches_than_the_ring_records(env):
    """20 launches round-robin over 3 (frames, out) pairs, each launch over
    another slice of its frames: an out ends up as its last launch left it.
    Then 20 launches into 20 different outs: no two conflict, so both lanes'
    rings (lanes.h LANE_RING = 8) overflow."""
    ctx, tbl = env
    n = 64 * 5
    f, o = ctx.refs.ref[(7 * n, 77)]
    exp = o["out"]
    fbs, obs = [], []
    for _ in range(3):
        fb = ctx.buffer(f.nbytes)
        fb.upload(f)
        fbs.append(fb)
        obs.append(ctx.buffer(4 * n))
        obs[-1].zero()
    for k in range(20):
        launch(ctx, tbl, fbs[k % 3].ptr + (k // 3) * n * 64, n, obs[k % 3].ptr)
    ctx.sync()
    for j in range(3):
        last = max(k for k in range(20) if k % 3 == j) // 3
        assert np.array_equal(obs[j].download(np.uint32, n), exp[last * n:(last + 1) * n]), j
    wide = ctx.buffer(4 * n * 20)
    wide.zero()
    for k in range(20):
        launch(ctx, tbl, fbs[0].ptr + (k % 7) * n * 64, n, wide.ptr + 4 * n * k)
    got = wide.download(np.uint32, 20 * n)
    for k in range(20):
        assert np.array_equal(got[k * n:(k + 1) * n], exp[(k % 7) * n:(k % 7 + 1) * n]), k
    for b in fbs + obs + [wide]:
        b.free()


def test_lane_entry_points_declared():
    """Bound, exported, and null handles refused before any device call (no GPU)."""
    assert "odpg_ctx_lanes" in L.SIGNATURES and "odpg_ctx_set_lanes" in L.SIGNATURES
    assert lib.odpg_ctx_lanes(None) == -22
    assert lib.odpg_ctx_set_lanes(None, 1) == -22


def test_lane_bookkeeping_against_model():
    """odp_amd/csrc/lanes.h (plain C) driven by tests/c/lanes_model.cpp, built
    with AddressSanitizer + UBSan and run as a plain executable: random
    launch / join sequences against a brute-force happens-before model."""
    import os
    import subprocess
    cdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c")
    r = subprocess.run(["make", "-s", "-C", cdir, "-f", "lanes_model.mk"], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([os.path.join(cdir, "lanes_model.asan")], capture_output=True, text=True,
                       timeout=300)
    out = r.stdout + r.stderr
    assert "ERROR: AddressSanitizer" not in out and "runtime error:" not in out, out[-4000:]
    assert r.returncode == 0 and "PASS: 4000 sequences" in r.stdout, out[-4000:]
    assert "ring of 5: 1000 launches" in r.stdout and "ring of 4: 1000 launches" in r.stdout
