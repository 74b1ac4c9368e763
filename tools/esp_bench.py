#!/usr/bin/env python3
"""Time odpg_esp() in both directions against a plain device copy of the same
bytes (DESIGN "ESP"). Three device-resident workloads, L3 offset 14:

  64    2^20 frames of 64 bytes at a fixed stride (a 50-byte inner IPv4 packet)
  imix  the C3 IMIX batch (2^20 frames by default), IPv4 and IPv6 inner frames
  1500  2^16 frames of 1500 bytes (descriptors, frames 1504 bytes apart)

each with AES-128 and AES-256 keys and with 1 and 1024 SAs (packet i uses SA
i mod 1024). The inbound plan decrypts what the outbound plan wrote.

  out_us, in_us  odpg_esp per call: device events around --calls back-to-back
                 calls after a warm-up of as many, --windows windows
  copy_us        hipMemcpyAsync device-to-device of the outbound total.bytes on
                 the same stream, measured the same way in alternating
                 windows: what a stage bound by HBM bandwidth would cost
  *_gbps         Gbit/s of inner-packet bytes

Prints one JSON line per case; median [min, max] over the windows. Before
anything is timed the round trip in(out(x)) is compared with the source frames
for a sample of packets. Needs a GPU: there is no fallback."""
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
L3 = 14


def fixed_batch(n, length, pitch):
    distinct = min(n, 1024)
    f = gen.ipv4_frames(distinct, length, gen.ip4("10.0.0.1"), gen.ip4("10.1.0.1"), gen.PROTO_UDP,
                        1000, 80)
    rows = np.zeros((distinct, pitch), np.uint8)
    rows[:, :length] = f
    desc = np.zeros(n, L.np_dtypes()[1])
    desc["offset"], desc["len"] = np.arange(n, dtype=np.uint64) * pitch, length
    return np.tile(rows, (n // distinct, 1)).reshape(-1), desc


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1 << 20, help="frames of 64 and imix")
    ap.add_argument("--big-batch", type=int, default=1 << 16, help="frames of 1500")
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--workloads", default="64,imix,1500")
    ap.add_argument("--keys", default="16,32")
    ap.add_argument("--sas", default="1,1024")
    args = ap.parse_args()
    desc_dt = L.np_dtypes()[1]
    ctx = gpu.Context(0)
    stream = lib.odpg_ctx_stream(ctx.h)
    rng = np.random.default_rng(5)
    for name in args.workloads.split(","):
        n = args.big_batch if name == "1500" else args.batch
        frames, desc = (gen.c3_frames(n) if name == "imix" else
                        fixed_batch(n, int(name), (int(name) + 15) // 16 * 16))
        cap = frames.nbytes + 80 * n
        fb, db = ctx.buffer(frames.nbytes + 64), ctx.buffer(desc.nbytes)
        eb, edb, pb, pdb = ctx.buffer(cap + 64), ctx.buffer(8 * n), ctx.buffer(cap + 64), ctx.buffer(8 * n)
        stb, sqb, tb, sab = ctx.buffer(n), ctx.buffer(4 * n), ctx.buffer(24), ctx.buffer(2 * n)
        fb.upload(frames)
        db.upload(desc)
        for key_len in map(int, args.keys.split(",")):
            for nsa in map(int, args.sas.split(",")):
                out, inb = ctx.esp(L.ESP_OUT, nsa, n), ctx.esp(L.ESP_IN, nsa, n)
                for k in range(nsa):
                    sa = L.esp_sa(0x100 + k, rng.bytes(key_len), rng.bytes(4), bytes([10, 0, 0, 1]),
                                  bytes([10, 0, 0, 2]))
                    out.set_sa(k, sa)
                    inb.set_sa(k, sa)
                sab.upload((np.arange(n) % nsa).astype("<u2"))
                sa_buf = sab if nsa > 1 else None

                def enc():
                    out.run_dev(fb, n, eb, cap, edb, n, stb, sqb, tb, desc_buf=db, sa_buf=sa_buf,
                                uniform_l3=L3)

                def dec():
                    inb.run_dev(eb, n, pb, cap, pdb, n, stb, sqb, tb, desc_buf=edb, sa_buf=sa_buf,
                                uniform_l3=L3)

                enc()
                ctx.sync()
                t_out = tb.download(np.dtype(L.ESP_TOTAL_FIELDS), 1)[0]
                ok_out, nbytes = int(t_out["num_out"]), int(t_out["bytes"])
                assert t_out["copied"] == n and nbytes <= cap, t_out
                dec()
                ctx.sync()
                t_in = tb.download(np.dtype(L.ESP_TOTAL_FIELDS), 1)[0]
                pdesc = pdb.download(desc_dt, n)
                assert t_in["num_out"] == ok_out > 0 and t_in["copied"] == n, (t_out, t_in)
                inner = int(pdesc["len"].sum()) - L3 * ok_out
                got = pb.download(np.uint8, int(t_in["bytes"]))
                for i in np.linspace(0, n - 1, 256).astype(np.int64):
                    o, (po, pl) = int(desc["offset"][i]), pdesc[i]
                    assert np.array_equal(got[po:po + pl], frames[o:o + pl]), ("round trip", i)

                cb = ctx.buffer(nbytes)

                def copy():
                    assert hip.hipMemcpyAsync(cb.ptr, eb.ptr, nbytes, D2D, stream) == 0

                # the three alternate, so all see the same neighbours
                t_e, t_d, t_c = [], [], []
                for _ in range(args.windows):
                    t_e += windows(ctx, enc, args.calls, 1)
                    t_d += windows(ctx, dec, args.calls, 1)
                    t_c += windows(ctx, copy, args.calls, 1)
                e, d, c = stat(t_e), stat(t_d), stat(t_c)
                print(json.dumps({"workload": name, "batch": n, "key_bits": 8 * key_len, "sas": nsa,
                                  "ok": ok_out, "inner_bytes": inner, "esp_bytes": nbytes,
                                  "calls": args.calls, "windows": args.windows, "out_us": e,
                                  "in_us": d, "copy_us": c, "out_ratio": round(e[0] / c[0], 1),
                                  "in_ratio": round(d[0] / c[0], 1),
                                  "out_gbps": round(8 * inner / e[0] / 1e3, 1),
                                  "in_gbps": round(8 * inner / d[0] / 1e3, 1)}), flush=True)
                cb.free()
                out.close()
                inb.close()
        for b in (fb, db, eb, edb, pb, pdb, stb, sqb, tb, sab):
            b.free()
    ctx.close()


if __name__ == "__main__":
    main()
