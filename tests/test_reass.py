"""IPv4 reassembly of a device-resident batch (include/odpg_reass.h).

Reference: parse() and reassemble() below, a plain restatement of the header's
rules 1-8 (a dict by flow, sorted, a loop, int.from_bytes), and expected(), the
layout and capacity rules. Bytes and integers are compared exactly. Every
output buffer is prefilled with 0xA5, so a stray write shows; the source
buffer's padding is random, so padding that is copied instead of zeroed shows.

A batch is a named scenario plus WHOLE UDP frames up to the size, in a fixed
random order. A scenario longer than one of the small sizes is cut to its
first `size` frames (its datagrams are then held); at the largest size the
batch grows in steps of 4 T until the scenario fits, so each one also runs
whole. T = the packets one workgroup of the copy kernel handles."""
import ctypes as C

import numpy as np
import pytest

from odp_amd import _lib as L
from odp_amd import gen

T = L.REASS_TILE
META_DT, DESC_DT = L.np_dtypes()
TOTAL_DT = np.dtype(L.REASS_TOTAL_FIELDS)
NO_L3 = L.OFFSET_INVALID
SIZES = [1, T - 1, T, T + 1, 4 * T + 3]
FILL32 = 0xA5A5A5A5


def parse(fr, l3):
    """None (WHOLE), "bad", or the fragment's fields."""
    n = len(fr)
    if l3 == NO_L3 or l3 + 20 > n or fr[l3] >> 4 != 4 or fr[l3] & 15 < 5 or l3 + 4 * (fr[l3] & 15) > n:
        return None
    f = int.from_bytes(fr[l3 + 6:l3 + 8], "big")
    mf, off = f & 0x2000, f & 0x1FFF
    if not mf and not off:
        return None
    hl, tl = 4 * (fr[l3] & 15), int.from_bytes(fr[l3 + 2:l3 + 4], "big")
    p = tl - hl
    if p <= 0 or l3 + tl > n or (mf and p % 8):
        return "bad"
    return dict(key=fr[l3 + 12:l3 + 20] + fr[l3 + 4:l3 + 6] + fr[l3 + 9:l3 + 10], start=8 * off,
                p=p, mf=mf, hl=hl, l3=l3, pay=fr[l3 + hl:l3 + tl])


def reassemble(pkts, l3s):
    """([(emitting index, origin, frame)] in output order, status, held)."""
    status, outs, groups = np.zeros(len(pkts), np.uint8), [], {}
    for i, (fr, l3) in enumerate(zip(pkts, l3s)):
        m = parse(fr, l3)
        if m is None:
            outs.append((i, i, fr))
        elif m == "bad":
            status[i] = L.REASS_BAD
        else:
            groups.setdefault(m["key"], []).append(dict(m, i=i))
    for ms in groups.values():
        ms.sort(key=lambda m: m["start"])
        m0, W = ms[0], ms[-1]["start"] + ms[-1]["p"]
        ok = (m0["start"] == 0 and all(a["start"] + a["p"] == b["start"] for a, b in zip(ms, ms[1:]))
              and all(m["mf"] for m in ms[:-1]) and not ms[-1]["mf"] and m0["hl"] + W <= 65535)
        for m in ms:
            status[m["i"]] = L.REASS_JOINED if ok else L.REASS_HELD
        if ok:
            l3, hl = m0["l3"], m0["hl"]
            fr = bytearray(pkts[m0["i"]][:l3 + hl] + b"".join(m["pay"] for m in ms))
            fr[l3 + 2:l3 + 4] = (hl + W).to_bytes(2, "big")
            fr[l3 + 6:l3 + 8] = bytes([fr[l3 + 6] & 0xC0, 0])
            fr[l3 + 10:l3 + 12] = b"\0\0"
            c = sum(int.from_bytes(fr[l3 + j:l3 + j + 2], "big") for j in range(0, hl, 2))
            c = (c & 0xFFFF) + (c >> 16)
            c = (c & 0xFFFF) + (c >> 16)
            fr[l3 + 10:l3 + 12] = (~c & 0xFFFF).to_bytes(2, "big")
            outs.append((max(m["i"] for m in ms), m0["i"], bytes(fr)))
    return sorted(outs), status, np.flatnonzero(status == L.REASS_HELD)


def expected(pkts, l3s, cap, max_out):
    """(frames[cap + 64], desc, origin, status, held, held_offsets, total) and the outputs."""
    outs, status, held_idx = reassemble(pkts, l3s)
    out = np.full(cap + 64, 0xA5, np.uint8)
    desc = np.full(max_out, FILL32, np.uint32).repeat(2).view(DESC_DT)
    origin, held = np.full(max_out, FILL32, np.uint32), np.full(len(pkts), FILL32, np.uint32)
    desc[:len(outs)] = (0, 0)
    origin[:len(outs)] = [o for _, o, _ in outs][:max_out]
    held[:len(held_idx)] = held_idx
    off = copied = 0
    for j, (_, _, fr) in enumerate(outs):
        al = (len(fr) + 15) // 16 * 16
        if j == copied and j < max_out and off + al <= cap:
            out[off:off + al] = 0
            out[off:off + len(fr)] = np.frombuffer(fr, np.uint8)
            desc[j] = (off, len(fr))
            copied += 1
        off += al
    total = np.array((len(outs), copied, len(held_idx), np.count_nonzero(status == L.REASS_BAD), off),
                     TOTAL_DT)
    return (out, desc, origin, status, held, np.array([0, len(held_idx)], np.uint32), total), outs


def pack(pkts, rng):
    """Frames 16-byte aligned in one buffer with random padding, and their descriptors."""
    desc = np.zeros(len(pkts), DESC_DT)
    desc["len"] = [len(p) for p in pkts]
    al = (desc["len"].astype(np.int64) + 15) // 16 * 16
    desc["offset"] = np.cumsum(al) - al
    buf = rng.integers(0, 256, int(al.sum()) + 64, np.uint8)
    for p, d in zip(pkts, desc):
        buf[d["offset"]:d["offset"] + d["len"]] = np.frombuffer(p, np.uint8)
    return buf, desc


def run_and_check(ctx, items, cap=None, max_out=None, stride=0, meta=False):
    """Reassemble on the GPU and compare every output with expected(); returns both."""
    pkts, l3s = [f for f, _ in items], [l3 for _, l3 in items]
    cap = sum((len(p) + 15) // 16 * 16 for p in pkts) if cap is None else cap
    max_out = len(pkts) if max_out is None else max_out
    ref, outs = expected(pkts, l3s, cap, max_out)
    l3, l3_stride = np.array(l3s, np.uint16), 2
    if meta:       # the u16 inside an odpg_meta_t array, as a classify result has it
        m = np.frombuffer(np.random.default_rng(3).bytes(len(pkts) * META_DT.itemsize), META_DT).copy()
        m["l3_offset"] = l3s
        l3, l3_stride = m.view(np.uint8)[META_DT.fields["l3_offset"][1]:].copy(), META_DT.itemsize
    plan = ctx.reass(len(pkts))        # tables at their densest
    if stride:
        got = plan.run(np.frombuffer(b"".join(pkts), np.uint8), int(l3s[0]), stride=stride,
                       capacity=cap, max_out=max_out, fill=0xA5)
    else:
        buf, desc = pack(pkts, np.random.default_rng(1))
        got = plan.run(buf, l3, desc=desc, capacity=cap, max_out=max_out, fill=0xA5,
                       l3_stride=l3_stride)
    plan.close()
    names = ("frames", "desc", "origin", "status", "held", "held_offsets", "total")
    for name, g, r in zip(names, got, ref):
        assert np.asarray(g).tobytes() == np.asarray(r).tobytes(), (name, g, r)
    return ref, outs, got


def ip(rng, flow, start, pay, mf, l2=14, ihl=5, tail=0, flags=0):
    """(frame, l3): l2 random bytes, an IPv4 header of flow (src, dst, id, proto) with random
    options, `pay` payload bytes at byte `start` of the datagram, `tail` bytes of padding."""
    h = bytearray(rng.bytes(4 * ihl))
    h[0] = 0x40 | ihl
    h[2:4] = (4 * ihl + pay).to_bytes(2, "big")
    h[4:6] = flow[2].to_bytes(2, "big")
    h[6:8] = ((0x2000 if mf else 0) | flags | start // 8).to_bytes(2, "big")
    h[9] = flow[3]
    h[12:20] = flow[0].to_bytes(4, "big") + flow[1].to_bytes(4, "big")
    return rng.bytes(l2) + bytes(h) + rng.bytes(pay) + rng.bytes(tail), l2


def datagram(rng, flow, sizes, **kw):
    """The fragments of one datagram with these payload sizes; kw[name] may be a list per member."""
    starts = np.cumsum([0] + list(sizes))
    return [ip(rng, flow, int(s), p, k < len(sizes) - 1,
               **{n: v[k] if isinstance(v, list) else v for n, v in kw.items()})
            for k, (s, p) in enumerate(zip(starts, sizes))]


def flow(k, ident=7, proto=17):
    return (0x0A000000 + k, 0x0A010000 + 3 * k, ident, proto)


def s_interleaved(rng):
    a = datagram(rng, flow(1), [24, 16, 8, 40, 13], tail=[0, 3, 0, 18, 7])[::-1]
    b = datagram(rng, flow(1, ident=8), [8] * 6 + [5])        # same addresses, another id
    b = [b[k] for k in rng.permutation(len(b))]
    return [x for pair in zip(a, b) for x in pair] + b[len(a):]


def s_incomplete(rng):
    d = [datagram(rng, flow(k), [16, 8, 24, 9]) for k in range(5)]
    overlap = [ip(rng, flow(9), 0, 16, True), ip(rng, flow(9), 8, 16, True), ip(rng, flow(9), 32, 8, False)]
    return (d[0][:1] + d[0][2:] + d[1][1:] + d[2] + [ip(rng, flow(2), 57, 3, False)] +
            d[3] + [d[3][1]] + overlap + d[4])                 # d[4] is complete


def s_headers(rng):
    """8-byte payloads land at 38 + 8 k (IHL 6) and 34 + 8 k: bytes 2, 6, 10 and 14 of a unit."""
    return (datagram(rng, flow(1), [8] * 9, ihl=[6] + [5] * 8, flags=0x4000) +
            datagram(rng, flow(2), [8] * 9, l2=[14, 18, 14, 18, 14, 18, 18, 14, 14], flags=0x8000) +
            datagram(rng, flow(3, proto=6), [64, 32, 100], ihl=[5, 15, 7], l2=[14, 22, 33]))


def s_nonfrag(rng):
    v6 = bytearray(rng.bytes(80))
    v6[14] = 0x60
    ihl4, cut = bytearray(ip(rng, flow(1), 8, 16, True)[0]), bytearray(ip(rng, flow(2), 8, 16, True, ihl=8)[0])
    ihl4[14] = 0x44
    return [(bytes(v6), 14), (ip(rng, flow(3), 8, 16, True)[0], NO_L3), (rng.bytes(33), 14), (b"", 14),
            (bytes(ihl4), 14), (bytes(cut[:40]), 14)] + datagram(rng, flow(4), [8, 8])


def s_bad(rng):
    good = datagram(rng, flow(1), [32, 32, 7])
    beyond = ip(rng, flow(1), 64, 40, False)                   # tot_len beyond the frame
    return good + [(beyond[0][:-1], 14), ip(rng, flow(1), 8, 0, True), ip(rng, flow(1), 8, 13, True),
                   (ip(rng, flow(2), 8, 16, True)[0], 0xFFF0)]


def s_big(rng):
    return datagram(rng, flow(1), [8] * 300)


def s_toolong(rng):
    return datagram(rng, flow(1), [32760, 32756]) + datagram(rng, flow(2), [32760, 32755])


def s_dense(rng):
    return [x for k in range(200) for x in datagram(rng, flow(k % 50, ident=k), [16, 9])]


def s_stride(rng):
    return [x for k in range(6) for x in datagram(rng, flow(k), [40, 88, 33][:2 + k % 2])]


SCENARIOS = {"interleaved": s_interleaved, "incomplete": s_incomplete, "headers": s_headers,
             "nonfrag": s_nonfrag, "bad": s_bad, "big300": s_big, "toolong": s_toolong,
             "dense": s_dense, "stride128": s_stride, "meta": s_interleaved}


def batch(name, size):
    rng = np.random.default_rng(1000 * sorted(SCENARIOS).index(name) + size)
    items, num = SCENARIOS[name](rng), size
    while size == SIZES[-1] and num < len(items):
        num += 4 * T
    items = items[:num] + [ip(rng, flow(100 + k), 0, 30 + k % 50, False) for k in range(num - len(items))]
    if name == "stride128":
        items = [(f + rng.bytes(128 - len(f)), l3) for f, l3 in items]
    return [items[k] for k in rng.permutation(num)]


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENARIOS)
def test_scenarios(gpu_ctx, name, size):
    ref, outs, _ = run_and_check(gpu_ctx, batch(name, size), stride=128 if name == "stride128" else 0,
                                 meta=name == "meta")
    if size == SIZES[-1]:      # the scenario ran whole: it did what its name says
        st, tot = ref[3], ref[6]
        want = {"interleaved": (12, 0, 0), "incomplete": (4, 19, 0), "headers": (21, 0, 0),
                "nonfrag": (2, 0, 0), "bad": (3, 0, 3), "big300": (300, 0, 0), "toolong": (2, 2, 0),
                "dense": (400, 0, 0), "stride128": (15, 0, 0), "meta": (12, 0, 0)}[name]
        assert (np.count_nonzero(st == L.REASS_JOINED), tot["num_held"], tot["num_bad"]) == want


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["short", "three", "max_out"])
def test_capacity(gpu_ctx, cut):
    """Capacity one byte short of the first output, exactly three outputs, and
    max_out below num_out: the copied prefix, {0, 0} descriptors, the fill
    beyond, total.bytes and num_out still the full need."""
    items = batch("interleaved", T + 1)
    outs = reassemble([f for f, _ in items], [l3 for _, l3 in items])[0]
    al = [(len(fr) + 15) // 16 * 16 for _, _, fr in outs]
    cap, max_out, copied = {"short": (al[0] - 1, len(outs), 0), "three": (sum(al[:3]), len(outs), 3),
                            "max_out": (sum(al), len(outs) - 2, len(outs) - 2)}[cut]
    ref, _, _ = run_and_check(gpu_ctx, items, cap=cap, max_out=max_out)
    assert ref[6]["copied"] == copied and ref[6]["bytes"] == sum(al) and ref[6]["num_out"] == len(outs)


@pytest.mark.gpu
def test_round_trip(gpu_ctx):
    """odpg_lso's IPv4 fragments (P = 64) in a fixed random order come back as
    the frames they were cut from, byte for byte; short frames pass through."""
    n = T + 5
    rows = [gen.ipv4_frames(n, ln, gen.ip4("10.0.0.1"), gen.ip4("10.1.0.1"), gen.PROTO_UDP, 5, 6,
                            ident=np.arange(n) + 1000 * k) for k, ln in enumerate((90, 300, 1001))]
    pkts = [bytes(r) for a in rows for r in a]
    rng = np.random.default_rng(5)
    buf, desc = pack(pkts, rng)
    lso = gpu_ctx.lso([L.lso_profile(L.LSO_PROTO_IPV4)], len(pkts))
    cap = 4 * buf.nbytes
    frames, sdesc, _, status, total = lso.run(buf, L.odpg_lso_opt_t(34, 64, 14, 0), desc=desc,
                                              capacity=cap, max_segs=20 * len(pkts))
    lso.close()
    assert not status.any() and total["copied"] == total["num_segs"] > 2 * len(pkts)
    segs = [bytes(frames[d["offset"]:d["offset"] + d["len"]]) for d in sdesc[:total["num_segs"]]]
    _, outs, _ = run_and_check(gpu_ctx, [(segs[k], 14) for k in rng.permutation(len(segs))])
    assert sorted(fr for _, _, fr in outs) == sorted(pkts)


@pytest.mark.gpu
def test_held_feeds_gather(gpu_ctx):
    """(held, held_offsets) is a one-bucket delivery list: odpg_gather of it
    yields the held frames in order."""
    items = batch("incomplete", SIZES[-1])
    ref, _, got = run_and_check(gpu_ctx, items)
    pkts = [f for f, _ in items]
    buf, desc = pack(pkts, np.random.default_rng(1))
    g = gpu_ctx.gather(len(pkts))
    frames, gdesc, _, total = g.run(buf, got[4], got[5], 0, 1, desc=desc)
    g.close()
    held = ref[4][:ref[6]["num_held"]]
    assert total["num"] == total["copied"] == len(held) > 0
    assert [bytes(frames[d["offset"]:d["offset"] + d["len"]]) for d in gdesc[:len(held)]] == \
        [pkts[i] for i in held]


BAD_ARGS = [(dict(num=101), {}), (dict(frames=None), {}), (dict(frames=8), {}),
            (dict(desc=None, stride=0), {}), (dict(desc=None, stride=72), {}),
            (dict(l3_offset=16, l3_stride=0), {}), (dict(l3_offset=16, l3_stride=3), {}),
            (dict(l3_offset=17), {}), ({}, dict(frames=None)), ({}, dict(frames=4)),
            ({}, dict(desc=None)), ({}, dict(origin=None)), ({}, dict(status=None)),
            ({}, dict(held=None)), ({}, dict(held_offsets=None)), ({}, dict(total=None)),
            ({}, dict(capacity=(1 << 32) + 1)), "plan", "src", "dst"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAD_ARGS, ids=str)
def test_arguments(gpu_ctx, case):
    """Every -EINVAL of the header returns before a launch: the outputs still
    hold their fill after a sync. An int stands for that offset into a buffer.
    An empty batch writes total and held_offsets only."""
    plan = gpu_ctx.reass(100)
    fb, ob = gpu_ctx.buffer(6400), gpu_ctx.buffer(6400)
    ob.upload(np.full(1600, FILL32, np.uint32))
    good_s = dict(frames=fb.ptr, desc=fb.ptr, stride=0, num=100, l3_offset=fb.ptr, l3_stride=2)
    good_d = dict(frames=ob.ptr, capacity=1024, desc=ob.ptr + 1024, max_out=10, origin=ob.ptr + 2048,
                  status=ob.ptr + 3072, held=ob.ptr + 4096, held_offsets=ob.ptr + 5120,
                  total=ob.ptr + 5136)
    ds, dd = case if isinstance(case, tuple) else ({}, {})
    fix = lambda base, d: {k: base + v if k in ("frames", "l3_offset") and v else v for k, v in d.items()}
    s = L.odpg_reass_src_t(**{**good_s, **fix(fb.ptr, ds)})
    d = L.odpg_reass_dst_t(**{**good_d, **fix(ob.ptr, dd)})
    args = [None if case == "plan" else plan.h, None if case == "src" else C.byref(s),
            None if case == "dst" else C.byref(d)]
    assert L.lib.odpg_reass(*args) == -22
    h = C.c_void_p()
    assert L.lib.odpg_reass_create(gpu_ctx.h, (1 << 24) + 1, C.byref(h)) == -22
    gpu_ctx.sync()
    assert np.all(ob.download(np.uint32, 1600) == FILL32)
    s, d = L.odpg_reass_src_t(**{**good_s, "num": 0}), L.odpg_reass_dst_t(**good_d)
    assert L.lib.odpg_reass(plan.h, C.byref(s), C.byref(d)) == 0
    gpu_ctx.sync()
    after = ob.download(np.uint32, 1600)
    assert after[1280:1282].tolist() == [0, 0] and after[1284:1290].tolist() == [0] * 6
    after[1280:1282] = after[1284:1290] = FILL32
    assert np.all(after == FILL32)
    plan.close()
    fb.free()
    ob.free()
