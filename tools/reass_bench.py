#!/usr/bin/env python3
"""Time odpg_reass() against a plain device copy of the same output bytes
(DESIGN "Reassembly"). Two device-resident workloads, both built on the
device by odpg_lso (IPv4 profile) and shuffled by odpg_gather with a fixed
random order:

  frags  2^16 UDP/IPv4 frames of 8814 bytes cut into 1480-byte payloads: six
         fragments each, every one part of a datagram that is complete
  imix   the C3 IMIX batch (2^20 frames by default) with every third
         unfragmented IPv4 frame of 570 or 1518 bytes (about 10 % of all
         frames) cut into 256-byte payloads; the rest pass through. The C3
         frames that carry MF already (0.5 % of its IPv4 frames) are held
         (570 bytes) or BAD (64 and 1518 bytes: MF with a payload that is
         no multiple of 8)

  reass_us  odpg_reass per call: device events around --calls back-to-back
            calls after a warm-up of as many, --windows windows
  copy_us   hipMemcpyAsync device-to-device of total.bytes on the same stream,
            measured the same way in alternating windows: the floor

Prints one JSON line per workload; median [min, max] over the windows. The
totals and a sample of outputs are checked against the frames the fragments
were cut from before anything is timed. Needs a GPU: there is no fallback."""
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
DESC_DT = L.np_dtypes()[1]
OPT_DT = np.dtype(L.LSO_OPT_FIELDS)


def frags_batch(n):
    """(frames, desc, options): n <= 2^16 frames, the IP id tells them apart"""
    assert n <= 1 << 16
    distinct = min(n, 1024)
    f = gen.ipv4_frames(distinct, 8814, gen.ip4("10.0.0.1"), gen.ip4("10.1.0.1"), gen.PROTO_UDP,
                        1000, 80)
    rows = np.zeros((n, 8816), np.uint8)
    rows[:, :8814] = np.tile(f, (n // distinct, 1))
    ident = np.arange(n)
    rows[:, 18], rows[:, 19], rows[:, 24:26] = ident >> 8, ident & 255, 0
    c = gen.csum(gen.ones_sum(rows, 14, 34))
    rows[:, 24], rows[:, 25] = c >> 8, c & 255
    desc = np.zeros(n, DESC_DT)
    desc["offset"], desc["len"] = np.arange(n, dtype=np.uint64) * 8816, 8814
    opts = np.zeros(n, OPT_DT)
    opts["payload_offset"], opts["max_payload_len"], opts["l3_offset"] = 34, 1480, 14
    return rows.reshape(-1), desc, opts


def imix_batch(n):
    frames, desc = gen.c3_frames(n)
    o = desc["offset"].astype(np.int64)
    plain4 = ((frames[o + 12] == 8) & (frames[o + 13] == 0) & ((frames[o + 20] & 0x3F) == 0) &
              (frames[o + 21] == 0) & (desc["len"] >= 570))
    cut = np.zeros(n, bool)
    cut[np.flatnonzero(plain4)[::3]] = True
    opts = np.zeros(n, OPT_DT)
    opts["payload_offset"], opts["l3_offset"] = 34, 14
    opts["max_payload_len"] = np.where(cut, 256, 0xFFF8)   # 0xFFF8: H + P > len, unchanged
    return frames, desc, opts


def flow_key(fr):
    return bytes(fr[26:34]) + bytes(fr[18:20]) + bytes(fr[23:24])


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--frags-batch", type=int, default=1 << 16)
    ap.add_argument("--imix-batch", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--workloads", default="frags,imix")
    args = ap.parse_args()
    ctx = gpu.Context(0)
    stream = lib.odpg_ctx_stream(ctx.h)
    for name in args.workloads.split(","):
        n = args.frags_batch if name == "frags" else args.imix_batch
        frames, desc, opts = (frags_batch if name == "frags" else imix_batch)(n)
        # fragment on the device, then shuffle the segments
        cap, max_segs = 2 * frames.nbytes, 8 * n
        lso = ctx.lso([L.lso_profile(L.LSO_PROTO_IPV4)], n)
        fb, db, ob = ctx.buffer(frames.nbytes + 64), ctx.buffer(desc.nbytes), ctx.buffer(opts.nbytes)
        sfb, sdb, sb, stb, tb = (ctx.buffer(cap + 64), ctx.buffer(8 * max_segs),
                                 ctx.buffer(4 * (n + 1)), ctx.buffer(n), ctx.buffer(24))
        for b, a in ((fb, frames), (db, desc), (ob, opts)):
            b.upload(a)
        lso.run_dev(fb, n, sfb, cap, sdb, max_segs, sb, stb, tb, desc_buf=db, opt_buf=ob)
        ctx.sync()
        total = tb.download(np.dtype(L.LSO_TOTAL_FIELDS), 1)[0]
        nseg, sbytes = int(total["num_segs"]), int(total["bytes"])
        assert total["copied"] == nseg <= max_segs and sbytes <= cap, total
        failed = int(np.count_nonzero(stb.download(np.uint8, n)))   # C3's IPv6 frames pass: rule 3
        order = np.random.default_rng(1).permutation(nseg).astype(np.uint32)
        gth = ctx.gather(nseg)
        rb, gob, gtb = ctx.buffer(4 * nseg), ctx.buffer(8), ctx.buffer(16)
        xfb, xdb = ctx.buffer(sbytes + 64), ctx.buffer(8 * nseg)
        rb.upload(order)
        gob.upload(np.array([0, nseg], np.uint32))
        gth.run_dev(sfb, nseg, rb, gob, 0, 1, xfb, sbytes, gtb, desc_buf=sdb, dst_desc_buf=xdb)
        ctx.sync()
        assert gtb.download(np.dtype(L.GATHER_TOTAL_FIELDS), 1)[0]["copied"] == nseg
        for b in (fb, db, ob, sfb, sdb, sb, stb, tb, rb, gob, gtb):
            b.free()
        lso.close()
        gth.close()

        plan = ctx.reass(nseg)
        rfb, rdb, rob = ctx.buffer(frames.nbytes + 64), ctx.buffer(8 * n), ctx.buffer(4 * n)
        rsb, rhb, rhob, rtb = ctx.buffer(nseg), ctx.buffer(4 * nseg), ctx.buffer(8), ctx.buffer(24)

        def reass():
            plan.run_dev(xfb, nseg, rfb, frames.nbytes, rdb, n, rob, rsb, rhb, rhob, rtb,
                         desc_buf=xdb, uniform_l3=14)

        reass()
        ctx.sync()
        tot = rtb.download(np.dtype(L.REASS_TOTAL_FIELDS), 1)[0]
        nout, nbytes = int(tot["num_out"]), int(tot["bytes"])
        assert tot["copied"] == nout <= n, tot
        if name == "frags":
            assert nout == n and tot["num_held"] == tot["num_bad"] == 0 and nbytes == frames.nbytes, tot
        rdesc = rdb.download(DESC_DT, nout)
        al = (rdesc["len"].astype(np.int64) + 15) // 16 * 16
        assert np.array_equal(rdesc["offset"], np.cumsum(al) - al), "layout"
        got = rfb.download(np.uint8, nbytes)
        # sampled outputs against the frames they were cut from (by flow key)
        src = {}
        for i in np.flatnonzero(opts["max_payload_len"] != 0xFFF8):
            o = int(desc["offset"][i])
            src[flow_key(frames[o:o + 34])] = (o, int(desc["len"][i]))
        joined = 0
        for j in np.linspace(0, nout - 1, 512).astype(np.int64):
            fr = got[rdesc["offset"][j]:rdesc["offset"][j] + rdesc["len"][j]]
            o, ln = src.get(flow_key(fr), (0, 0)) if len(fr) >= 34 else (0, 0)
            if ln == len(fr) and ln > 290:     # a frame LSO did cut
                want = frames[o:o + ln].copy()
                want[24:26] = fr[24:26]        # C3 has frames with a wrong header checksum
                assert np.array_equal(fr, want), ("output", j)
                joined += 1
        assert joined > 16, joined

        cb = ctx.buffer(nbytes)

        def copy():
            assert hip.hipMemcpyAsync(cb.ptr, rfb.ptr, nbytes, D2D, stream) == 0

        # the two alternate, so both see the same neighbours
        t_r, t_c = [], []
        for _ in range(args.windows):
            t_r += windows(ctx, reass, args.calls, 1)
            t_c += windows(ctx, copy, args.calls, 1)
        g, c = stat(t_r), stat(t_c)
        print(json.dumps({"workload": name, "source_frames": n, "lso_failed": failed, "batch": nseg,
                          "src_bytes": sbytes, "outputs": nout, "held": int(tot["num_held"]), "bad": int(tot["num_bad"]),
                          "bytes": nbytes, "sampled_joined": joined, "calls": args.calls,
                          "windows": args.windows, "reass_us": g, "copy_us": c,
                          "ratio": round(g[0] / c[0], 2),
                          "reass_GBps_rw": round(2 * nbytes / g[0] / 1e3, 1)}), flush=True)
        for b in (xfb, xdb, rfb, rdb, rob, rsb, rhb, rhob, rtb, cb):
            b.free()
        plan.close()
    ctx.close()


if __name__ == "__main__":
    main()
