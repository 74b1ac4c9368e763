#!/usr/bin/env python3
"""Time odpg_lso() against a plain device copy of the same bytes (DESIGN
"segmentation offload"). Two device-resident workloads:

  tso   2^16 TCP/IPv4 frames of 54 + 8760 bytes (descriptors, frames 8816
        bytes apart), custom profile (IP id and TCP sequence number by
        ADD_SEGMENT_NUM), H = 54, P = 1460: six segments of 1514 bytes each
  imix  the C3 IMIX batch (2^20 frames by default), IPv4 profile, H = 34,
        P = 552, l3 = 14: 64- and 570-byte frames pass unchanged, 1518-byte
        IPv4 frames become three fragments, 1518-byte IPv6 frames fail
        (BAD_IHL) and produce nothing

  lso_us   odpg_lso per call: device events around --calls back-to-back calls
           after a warm-up of as many, --windows windows
  copy_us  hipMemcpyAsync device-to-device of total.bytes on the same stream,
           measured the same way in alternating windows: the floor

Prints one JSON line per workload; median [min, max] over the windows. The
totals and a sample of segments are checked before anything is timed. Needs
a GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odp_amd import _lib as L          # noqa: E402
from odp_amd import gen, gpu           # noqa: E402
from deliver_bench import stat, windows   # noqa: E402

lib = L.lib
hip = C.CDLL("libamdhip64.so")
hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
lib.odpg_ctx_stream.restype = C.c_void_p
D2D = 3   # hipMemcpyDeviceToDevice


def tso_batch(n):
    distinct = min(n, 1024)
    f = gen.ipv4_frames(distinct, 54 + 8760, gen.ip4("10.0.0.1"), gen.ip4("10.1.0.1"),
                        gen.PROTO_TCP, 1000, 80)
    rows = np.zeros((distinct, 8816), np.uint8)
    rows[:, :8814] = f
    desc = np.zeros(n, L.np_dtypes()[1])
    desc["offset"], desc["len"] = np.arange(n, dtype=np.uint64) * 8816, 8814
    profile = L.lso_profile(L.LSO_PROTO_CUSTOM, [(L.LSO_ADD_SEGMENT_NUM, 18, 2),
                                                 (L.LSO_ADD_SEGMENT_NUM, 38, 4)])
    return (np.tile(rows, (n // distinct, 1)).reshape(-1), desc, profile,
            L.odpg_lso_opt_t(54, 1460, L.OFFSET_INVALID, 0))


def imix_batch(n):
    frames, desc = gen.c3_frames(n)
    return frames, desc, L.lso_profile(L.LSO_PROTO_IPV4), L.odpg_lso_opt_t(34, 552, 14, 0)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--tso-batch", type=int, default=1 << 16)
    ap.add_argument("--imix-batch", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--workloads", default="tso,imix")
    args = ap.parse_args()
    desc_dt = L.np_dtypes()[1]
    ctx = gpu.Context(0)
    stream = lib.odpg_ctx_stream(ctx.h)
    for name in args.workloads.split(","):
        n = args.tso_batch if name == "tso" else args.imix_batch
        frames, desc, profile, uniform = (tso_batch if name == "tso" else imix_batch)(n)
        H, P = uniform.payload_offset, uniform.max_payload_len
        cap, max_segs = 2 * frames.nbytes, 8 * n
        plan = ctx.lso([profile], n)
        fb, db, gfb = ctx.buffer(frames.nbytes + 64), ctx.buffer(desc.nbytes), ctx.buffer(cap + 64)
        gdb, sb, stb, tb = (ctx.buffer(8 * max_segs), ctx.buffer(4 * (n + 1)), ctx.buffer(n),
                            ctx.buffer(24))
        fb.upload(frames)
        db.upload(desc)

        def lso():
            plan.run_dev(fb, n, gfb, cap, gdb, max_segs, sb, stb, tb, desc_buf=db, uniform=uniform)

        lso()
        ctx.sync()
        total = tb.download(np.dtype(L.LSO_TOTAL_FIELDS), 1)[0]
        nseg, nbytes = int(total["num_segs"]), int(total["bytes"])
        assert total["copied"] == nseg <= max_segs and nbytes <= cap, total
        first, status = sb.download(np.uint32, n + 1), stb.download(np.uint8, n)
        gdesc = gdb.download(desc_dt, nseg)
        al = (gdesc["len"].astype(np.int64) + 15) // 16 * 16
        assert first[n] == nseg and np.array_equal(gdesc["offset"], np.cumsum(al) - al), "layout"
        got = gfb.download(np.uint8, nbytes)
        # payloads of sampled packets, reassembled from their segments
        for i in np.linspace(0, n - 1, 256).astype(np.int64):
            o, ln = int(desc["offset"][i]), int(desc["len"][i])
            segs = [got[d["offset"]:d["offset"] + d["len"]] for d in gdesc[first[i]:first[i + 1]]]
            if status[i]:
                assert not segs, ("failed packet", i)
            elif len(segs) == 1:
                assert np.array_equal(segs[0], frames[o:o + ln]), ("unchanged", i)
            else:
                assert np.array_equal(np.concatenate([s[H:] for s in segs]),
                                      frames[o + H:o + ln]), ("payload", i)

        cb = ctx.buffer(nbytes)

        def copy():
            assert hip.hipMemcpyAsync(cb.ptr, gfb.ptr, nbytes, D2D, stream) == 0

        # the two alternate, so both see the same neighbours
        t_l, t_c = [], []
        for _ in range(args.windows):
            t_l += windows(ctx, lso, args.calls, 1)
            t_c += windows(ctx, copy, args.calls, 1)
        g, c = stat(t_l), stat(t_c)
        print(json.dumps({"workload": name, "batch": n, "H": H, "P": P, "segments": nseg,
                          "failed": int(np.count_nonzero(status)), "src_bytes": int(desc["len"].sum()),
                          "bytes": nbytes, "calls": args.calls, "windows": args.windows,
                          "lso_us": g, "copy_us": c, "ratio": round(g[0] / c[0], 2),
                          "lso_GBps_rw": round(2 * nbytes / g[0] / 1e3, 1)}), flush=True)
        for b in (fb, db, gfb, gdb, sb, stb, tb, cb):
            b.free()
        plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
