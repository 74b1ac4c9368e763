#!/usr/bin/env python3
"""Time odpg_gather() against a plain device copy of the same bytes (DESIGN
"dense queue batches"). Per traffic mix at --batch packets, device-resident,
after classify -> deliver of the batch, gathering all delivered buckets
[0, B - 2):

  gather_us   odpg_gather per call: device events around --calls back-to-back
              calls after a warm-up, --windows windows
  copy_us     hipMemcpyAsync device-to-device of total.bytes on the same
              stream, measured the same way in the same session: the floor
  deliver_us  odpg_deliver of the batch, for scale

c2: C2 frames, fixed stride 64 (one launch). c3: C3 IMIX frames with
descriptors (three launches). Prints one JSON line per mix; median [min, max]
over the windows. The gathered batch is checked against numpy before anything
is timed. Needs a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odp_amd import _lib as L          # noqa: E402
from odp_amd import cls, gen, gpu      # noqa: E402
from deliver_bench import stat, windows   # noqa: E402

lib = L.lib
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
lib.odpg_ctx_stream.restype = C.c_void_p
D2D = 3   # hipMemcpyDeviceToDevice


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--configs", default="c2,c3")
    args = ap.parse_args()
    n = args.batch
    opt = L.PKTIN_IPV4_CHKSUM | L.PKTIN_UDP_CHKSUM | L.PKTIN_TCP_CHKSUM
    desc_dt = L.np_dtypes()[1]
    ctx = gpu.Context(0)
    stream = lib.odpg_ctx_stream(ctx.h)
    for config in args.configs.split(","):
        cls.reset()
        pktio = cls.loop_pktio(pktin=opt)
        (gen.build_c3_rules if config == "c3" else gen.build_c2_rules)(cls, pktio)
        assert cls.pktio_start(pktio) == 0
        tbl = ctx.table(cls.pktio_rules(pktio))
        dplan, gplan = ctx.deliver(tbl, n), ctx.gather(n)
        B = dplan.num_buckets
        if config == "c3":
            (frames, desc), stride = gen.c3_frames(n), 0
        else:
            frames, desc, stride = gen.c2_frames(n), None, 64
        cap = frames.nbytes
        fb, gfb = ctx.buffer(cap + 64), ctx.buffer(cap + 64)
        db, gdb = ctx.buffer(8 * n), ctx.buffer(8 * n)
        ob, gwb, rb = ctx.buffer(4 * n), ctx.buffer(4 * n), ctx.buffer(4 * n)
        sb, tb = ctx.buffer(4 * (B + 1)), ctx.buffer(16)
        fb.upload(frames)
        if desc is not None:
            db.upload(desc)
        sdesc = db if desc is not None else None

        def deliver():
            dplan.run_dev(ob, n, rb, sb)

        def gather():
            gplan.run_dev(fb, n, rb, sb, 0, B - 2, gfb, cap, tb, stride, sdesc, ob, gdb, gwb)

        ctx.classify_dev(tbl, fb, n, stride=stride, desc_buf=sdesc, opt=opt, out_buf=ob)
        deliver()
        gather()
        ctx.sync()
        total = tb.download(np.dtype(L.GATHER_TOTAL_FIELDS), 1)[0]
        order, offsets = rb.download(np.uint32, n), sb.download(np.uint32, B + 1)
        m, nbytes = int(offsets[B - 2]), int(total["bytes"])
        assert total["num"] == total["copied"] == m and nbytes <= cap, total
        idx = order[:m]
        assert np.array_equal(gwb.download(np.uint32, m), ob.download(np.uint32, n)[idx]), "words"
        got, gdesc = gfb.download(np.uint8, nbytes), gdb.download(desc_dt, m)
        if desc is None:
            assert nbytes == 64 * m and np.array_equal(got.reshape(m, 64),
                                                       frames.reshape(n, 64)[idx]), "frames"
        else:
            ln = desc["len"][idx].astype(np.int64)
            al = (ln + 15) // 16 * 16
            off = np.cumsum(al) - al
            assert nbytes == al.sum() and np.array_equal(gdesc["offset"], off), "offsets"
            assert np.array_equal(gdesc["len"], ln), "lengths"
            for j in np.linspace(0, m - 1, 512).astype(np.int64):
                s = int(desc["offset"][idx[j]])
                assert np.array_equal(got[off[j]:off[j] + ln[j]], frames[s:s + ln[j]]), ("frame", j)
                assert not np.any(got[off[j] + ln[j]:off[j] + al[j]]), ("padding", j)

        def copy():
            assert hip.hipMemcpyAsync(gfb.ptr, fb.ptr, nbytes, D2D, stream) == 0

        # gather and the copy alternate, so both see the same neighbours
        t_g, t_c = [], []
        for _ in range(args.windows):
            t_g += windows(ctx, gather, args.calls, 1)
            t_c += windows(ctx, copy, args.calls, 1)
        t_d = windows(ctx, deliver, args.calls, args.windows)
        g, c = stat(t_g), stat(t_c)
        print(json.dumps({"config": config, "batch": n, "buckets": B, "gathered": m,
                          "bytes": nbytes, "calls": args.calls, "windows": args.windows,
                          "gather_us": g, "copy_us": c, "ratio": round(g[0] / c[0], 2),
                          "gather_GBps_rw": round(2 * nbytes / g[0] / 1e3, 1),
                          "deliver_us": stat(t_d)}), flush=True)
        for b in (fb, gfb, db, gdb, ob, gwb, rb, sb, tb):
            b.free()
        dplan.close()
        gplan.close()
        del tbl
    ctx.close()
    cls.reset()


if __name__ == "__main__":
    main()
