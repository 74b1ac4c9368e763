#!/usr/bin/env python3
"""Time odpg_deliver() against the host path it replaces (DESIGN "delivery
lists"). Per table (C2, C4 of bench.py) at --batch packets, device-resident:

  deliver_us    odpg_deliver per call: device events around --calls
                back-to-back calls after a warm-up, --windows windows
  classify_us   odpg_classify of the same batch, measured the same way
  d2h_us        odpg_memcpy_d2h of the verdict words (host clock, the call
                ends in a stream synchronise)
  host_us       a single-threaded numpy pass over the copied words that
                builds the same lists (bucket rule, stable argsort, bincount)

Prints one JSON line per table; median [min, max] over the windows. The
device lists are checked against the numpy ones before anything is timed.
Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odp_amd import _lib as L          # noqa: E402
from odp_amd import cls, gen, gpu      # noqa: E402

lib = L.lib


def host_lists(words, qb, nc, B):
    w = words.astype(np.int64)
    c, q = w & 0xFFFF, (w >> 24) & 31
    ci = np.minimum(c, nc - 1)
    ok = (c < nc) & ((w & L.ODPG_OUT_CLS_DROP) == 0) & (q < qb[ci + 1] - qb[ci])
    b = np.where(ok, qb[ci] + q, np.where(c == L.ODPG_COS_NOCLS, B - 2, B - 1))
    return (np.argsort(b, kind="stable").astype(np.uint32),
            np.concatenate([[0], np.cumsum(np.bincount(b, minlength=B))]).astype(np.uint32))


def windows(ctx, fn, calls, nwin):
    """per-call microseconds of `fn`, one figure per window of `calls`"""
    for _ in range(calls):
        fn()
    ctx.sync()
    out, ms = [], C.c_float()
    for _ in range(nwin):
        L.check(lib.odpg_event_record(ctx.h, 0), "event")
        for _ in range(calls):
            fn()
        L.check(lib.odpg_event_record(ctx.h, 1), "event")
        L.check(lib.odpg_event_elapsed_ms(ctx.h, 0, 1, C.byref(ms)), "elapsed")
        out.append(ms.value * 1e3 / calls)
    return out


def stat(v):
    return [round(float(np.median(v)), 2), round(float(min(v)), 2), round(float(max(v)), 2)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    n = args.batch
    opt = L.PKTIN_IPV4_CHKSUM | L.PKTIN_UDP_CHKSUM | L.PKTIN_TCP_CHKSUM
    ctx = gpu.Context(0)
    for config in ("c2", "c4"):
        cls.reset()
        if config == "c4":
            assert cls.set_limits(2048, 2048, 32) == 0
        pktio = cls.loop_pktio(pktin=opt)
        (gen.build_c4_rules if config == "c4" else gen.build_c2_rules)(cls, pktio)
        assert cls.pktio_start(pktio) == 0
        tbl = ctx.table(cls.pktio_rules(pktio))
        plan = ctx.deliver(tbl, n)
        B, nc = plan.num_buckets, plan.num_cos
        qb = np.array([plan.queue_base(c) for c in range(nc)] + [B - 2], np.int64)
        frames = gen.c2_frames(n)
        fb, ob = ctx.buffer(frames.nbytes + 64), ctx.buffer(4 * n)
        rb, sb = ctx.buffer(4 * n), ctx.buffer(4 * (B + 1))
        fb.upload(frames)

        def classify():
            ctx.classify_dev(tbl, fb, n, stride=64, opt=opt, out_buf=ob)

        def deliver():
            plan.run_dev(ob, n, rb, sb)

        classify()
        deliver()
        ctx.sync()
        words = ob.download(np.uint32, n)
        order, offsets = host_lists(words, qb, nc, B)
        assert np.array_equal(rb.download(np.uint32, n), order), "order differs from numpy"
        assert np.array_equal(sb.download(np.uint32, B + 1), offsets), "offsets differ"
        t_cls = windows(ctx, classify, args.calls, args.windows)
        t_dlv = windows(ctx, deliver, args.calls, args.windows)
        t_d2h, t_host = [], []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            words = ob.download(np.uint32, n)
            t1 = time.perf_counter()
            host_lists(words, qb, nc, B)
            t2 = time.perf_counter()
            t_d2h.append((t1 - t0) * 1e6)
            t_host.append((t2 - t1) * 1e6)
        bits = max(1, int(B - 1).bit_length())
        print(json.dumps({"config": config, "batch": n, "buckets": B,
                          "passes": 1 if bits <= 11 else 2, "calls": args.calls,
                          "windows": args.windows, "deliver_us": stat(t_dlv),
                          "classify_us": stat(t_cls), "d2h_us": stat(t_d2h),
                          "host_us": stat(t_host)}), flush=True)
        for b in (fb, ob, rb, sb):
            b.free()
        plan.close()
        del tbl
    ctx.close()
    cls.reset()


if __name__ == "__main__":
    main()
