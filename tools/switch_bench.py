#!/usr/bin/env python3
"""Time odpg_switch() on device-resident batches (DESIGN "L2 switch"). Two
workloads of --batch (2^20) frames of 64 bytes on 8 ports, source and
destination uniformly random among the hosts, a host's port fixed:

  hosts1k    1024 hosts: few slot collisions, writer runs of about 1024
  hosts128k  2^17 hosts: most slots shared by several MACs, runs of about 8

  switch_us    odpg_switch per call: device events around --calls back-to-back
               calls after a warm-up of as many, --windows windows
  classify_us  odpg_classify (verdict only, the C4 table) of the same frames
  deliver_us   odpg_deliver of as many verdict words (C4: two radix passes)
  d2h_us       a device-to-host copy of 16 bytes per packet: the round trip
               of the address bytes a host-side MAC table would need

The three yardsticks run their own existing code in the same session. Prints
one JSON line per workload; median [min, max] over the windows. The first call
(on the zeroed table) is checked whole against the sequential loop on the
host before anything is timed. Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from odp_amd import _lib as L          # noqa: E402
from odp_amd import cls, gen, gpu      # noqa: E402
from deliver_bench import stat, windows   # noqa: E402

PORTS = 8


def crc_tables():
    """tab[k][b]: CRC32C (initial value 0) of six bytes, b at position k, the others zero"""
    x, tab = np.arange(256, dtype=np.uint32), np.zeros((6, 256), np.uint32)
    for k in range(5, -1, -1):
        for _ in range(8):
            x = (x >> 1) ^ np.where(x & 1, np.uint32(0x82F63B78), np.uint32(0))
        tab[k] = x
    return tab


def slots(macs, tab):
    s = np.zeros(len(macs), np.uint32)
    for k in range(6):
        s ^= tab[k][macs[:, k]]
    return s & 0xFFFF


def host_switch(frames, ports, tick):
    """out words and totals of the batch on a zeroed table (every frame valid, no broadcast)"""
    tab = crc_tables()
    ds, ss = slots(frames[:, 0:6], tab).tolist(), slots(frames[:, 6:12], tab).tolist()
    pad = np.zeros((len(frames), 2), np.uint8)
    dm = np.concatenate([frames[:, 0:6], pad], 1).view("<u8").ravel().tolist()
    sm = np.concatenate([frames[:, 6:12], pad], 1).view("<u8").ravel().tolist()
    table, out, entries = {}, np.empty(len(frames), np.uint32), 0
    for i, p in enumerate(ports.tolist()):
        table[ss[i]] = (sm[i], p)
        mac, q = table.get(ds[i], (0, 0))
        out[i] = q if mac == dm[i] else L.SWITCH_FLOOD << 8
        entries += 1 if mac == dm[i] else PORTS - 1
    uni = int(np.count_nonzero(out < 256))
    return out, (uni, len(frames) - uni, 0, entries)


def batch(n, hosts, seed):
    rng = np.random.default_rng(seed)
    macs = np.zeros((hosts, 6), np.uint8)
    macs[:, 0] = 2
    macs[:, 2:6] = rng.integers(0, 256, (hosts, 4), np.uint8)
    d, s = rng.integers(0, hosts, n), rng.integers(0, hosts, n)
    frames = gen.c2_frames(n).reshape(n, 64).copy()
    frames[:, 0:6], frames[:, 6:12] = macs[d], macs[s]
    return frames, (s % PORTS).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=1 << 20)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--windows", type=int, default=9)
    args = ap.parse_args()
    n = args.batch
    opt = L.PKTIN_IPV4_CHKSUM | L.PKTIN_UDP_CHKSUM | L.PKTIN_TCP_CHKSUM
    ctx = gpu.Context(0)
    cls.reset()
    assert cls.set_limits(2048, 2048, 32) == 0
    pktio = cls.loop_pktio(pktin=opt)
    gen.build_c4_rules(cls, pktio)
    assert cls.pktio_start(pktio) == 0
    tbl = ctx.table(cls.pktio_rules(pktio))
    dlv = ctx.deliver(tbl, n)
    for name, hosts in (("hosts1k", 1 << 10), ("hosts128k", 1 << 17)):
        frames, ports = batch(n, hosts, hosts)
        plan = ctx.switch(PORTS, n)
        fb, pb, ob = ctx.buffer(frames.nbytes + 64), ctx.buffer(n), ctx.buffer(4 * n)
        lb, fo, tb = ctx.buffer(4 * PORTS * n), ctx.buffer(8 * PORTS), ctx.buffer(16)
        vb, rb, sb = ctx.buffer(4 * n), ctx.buffer(4 * n), ctx.buffer(4 * (dlv.num_buckets + 1))
        ab = ctx.buffer(16 * n)
        fb.upload(frames)
        pb.upload(ports)

        def switch():
            plan.run_dev(fb, n, 1, ob, lb, n, fo, tb, stride=64, port_in_buf=pb)

        def classify():
            ctx.classify_dev(tbl, fb, n, stride=64, opt=opt, out_buf=vb)

        def deliver():
            dlv.run_dev(vb, n, rb, sb)

        switch()
        classify()
        ctx.sync()
        want, total = host_switch(frames, ports, 1)
        assert np.array_equal(ob.download(np.uint32, n), want), "out differs from the host loop"
        got = tb.download(np.dtype(L.SWITCH_TOTAL_FIELDS), 1)[0]
        assert tuple(int(v) for v in got) == total, (got, total)
        counts = fo.download(np.uint32, 2 * PORTS)[1::2]
        assert int(counts.sum()) == total[3]
        used = int(np.count_nonzero(plan.table()))
        t_sw = windows(ctx, switch, args.calls, args.windows)
        t_cls = windows(ctx, classify, args.calls, args.windows)
        t_dlv = windows(ctx, deliver, args.calls, args.windows)
        t_d2h = []
        for _ in range(args.windows):
            t0 = time.perf_counter()
            ab.download(np.uint8, 16 * n)
            t_d2h.append((time.perf_counter() - t0) * 1e6)
        print(json.dumps({"workload": name, "batch": n, "hosts": hosts, "ports": PORTS,
                          "slots_used": used, "first_call": dict(zip(got.dtype.names, total)),
                          "calls": args.calls, "windows": args.windows, "switch_us": stat(t_sw),
                          "classify_us": stat(t_cls), "deliver_us": stat(t_dlv),
                          "d2h_us": stat(t_d2h)}), flush=True)
        for b in (fb, pb, ob, lb, fo, tb, vb, rb, sb, ab):
            b.free()
        plan.close()
    dlv.close()
    del tbl
    ctx.close()
    cls.reset()


if __name__ == "__main__":
    main()
