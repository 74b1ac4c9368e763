"""Segmentation offload of a device-resident batch (include/odpg_lso.h).

Reference: segment() below, a plain restatement of the header's rules (a loop
per packet and per segment, int.from_bytes), and expected(), the layout and
capacity rules. Bytes and integers are compared exactly. Every output buffer
is prefilled with 0xA5, so a write outside the segments shows; the source
buffer's padding is random, so padding that is copied instead of zeroed shows.
T = the packets one workgroup of the copy kernel handles; there is no other
threshold in the work split."""
import ctypes as C

import numpy as np
import pytest

import oracle
from helpers import has
from odp_amd import _lib as L
from odp_amd import gen

T = L.LSO_TILE
DESC_DT = L.np_dtypes()[1]
OPT_DT, TOTAL_DT = np.dtype(L.LSO_OPT_FIELDS), np.dtype(L.LSO_TOTAL_FIELDS)
IPV4, CUSTOM, ADD, BITS = L.LSO_PROTO_IPV4, L.LSO_PROTO_CUSTOM, L.LSO_ADD_SEGMENT_NUM, L.LSO_WRITE_BITS
NO_L3 = L.OFFSET_INVALID
SEQ16 = (CUSTOM, [(ADD, 16, 2)])       # the reference test's custom profile (lso.c:655-660)
PROFILES = [SEQ16, (IPV4, [])]


def segment(fr, H, P, l3, prof, profiles):
    """(status, [segment bytes]) of one frame."""
    if prof >= len(profiles):
        return L.LSO_BAD_PROFILE, []
    if H > 128 or H > len(fr):
        return L.LSO_BAD_OFFSET, []
    if H + P > len(fr):
        return 0, [fr]
    proto, fields = profiles[prof]
    if proto == IPV4:
        if l3 == NO_L3 or H < l3 or H - l3 < 20:
            return L.LSO_BAD_L3, []
        P = P // 8 * 8
    if P == 0:
        return L.LSO_BAD_PAYLOAD, []
    n, left = divmod(len(fr) - H, P)
    n += left != 0
    if n > 64:
        return L.LSO_TOO_MANY, []
    if n == 1:
        return 0, [fr]
    out = []
    for k in range(n):
        s = bytearray(fr[:H] + fr[H + k * P:H + k * P + P])
        if proto == IPV4:
            if s[l3] & 15 != 5:
                return L.LSO_BAD_IHL, []
            frag = (int.from_bytes(s[l3 + 6:l3 + 8], "big") + k * P // 8) & 0xFFFF
            s[l3 + 2:l3 + 4] = ((len(s) - l3) & 0xFFFF).to_bytes(2, "big")
            s[l3 + 6:l3 + 8] = (frag | (0x2000 if k < n - 1 else 0)).to_bytes(2, "big")
            s[l3 + 10:l3 + 12] = b"\0\0"
            c = sum(int.from_bytes(s[l3 + j:l3 + j + 2], "big") for j in range(0, 20, 2))
            c = (c & 0xFFFF) + (c >> 16)
            c = (c & 0xFFFF) + (c >> 16)
            s[l3 + 10:l3 + 12] = (~c & 0xFFFF).to_bytes(2, "big")
        for op, off, size, *bits in fields:
            if off + size > len(s):
                return L.LSO_BAD_FIELD, []
            v = int.from_bytes(s[off:off + size], "big")
            if op == ADD:
                v = (v + k) % (1 << 8 * size)
            else:
                m, val = bits[0 if k == 0 else 2 if k == n - 1 else 1]
                v = (v & ~m) | (val & m)
            s[off:off + size] = v.to_bytes(size, "big")
        out.append(bytes(s))
    return 0, out


def expected(pkts, opts, profiles, cap, max_segs):
    """(frames[cap + 64], desc[max_segs], seg_first, status, total) and the segments."""
    res = [segment(fr, int(o["payload_offset"]), int(o["max_payload_len"]), int(o["l3_offset"]),
                   int(o["profile"]), profiles) for fr, o in zip(pkts, opts)]
    status = np.array([st for st, _ in res], np.uint8)
    seg_first = np.cumsum([0] + [len(s) for _, s in res]).astype(np.uint32)
    segs = [s for _, ss in res for s in ss]
    out = np.full(cap + 64, 0xA5, np.uint8)
    desc = np.full(max_segs, 0xA5A5A5A5, np.uint32).repeat(2).view(DESC_DT)
    desc[:len(segs)] = (0, 0)
    off = copied = 0
    for j, s in enumerate(segs):
        al = (len(s) + 15) // 16 * 16
        if j == copied and j < max_segs and off + al <= cap:
            out[off:off + al] = 0
            out[off:off + len(s)] = np.frombuffer(s, np.uint8)
            desc[j] = (off, len(s))
            copied += 1
        off += al
    bad = np.flatnonzero(status)
    total = np.array((len(segs), copied, bad[0] if len(bad) else len(pkts), 0, off), TOTAL_DT)
    return (out, desc, seg_first, status, total), segs


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


def opt_array(rows):
    o = np.zeros(len(rows), OPT_DT)
    for r, (H, P, l3, prof) in zip(o, rows):
        r["payload_offset"], r["max_payload_len"], r["l3_offset"], r["profile"] = H, P, l3, prof
    return o


def run_and_check(ctx, profiles, pkts, rows, cap=None, max_segs=None, uniform=False, stride=0,
                  seed=1):
    """Segment on the GPU and compare every output with expected(); returns the reference."""
    opts = opt_array(rows)
    if cap is None:
        cap = sum((len(p) + 15) // 16 * 16 + 16 * 64 for p in pkts)
    max_segs = 64 * len(pkts) if max_segs is None else max_segs
    ref, segs = expected(pkts, opts, profiles, cap, max_segs)
    plan = ctx.lso([L.lso_profile(*p) for p in profiles], len(pkts))
    arg = L.odpg_lso_opt_t(*rows[0]) if uniform else opts
    if stride:
        got = plan.run(np.frombuffer(b"".join(pkts), np.uint8), arg, stride=stride, capacity=cap,
                       max_segs=max_segs, fill=0xA5)
    else:
        buf, desc = pack(pkts, np.random.default_rng(seed))
        got = plan.run(buf, arg, desc=desc, capacity=cap, max_segs=max_segs, fill=0xA5)
    plan.close()
    for name, g, r in zip(("frames", "desc", "seg_first", "status", "total"), got, ref):
        assert np.asarray(g).tobytes() == np.asarray(r).tobytes(), (name, g, r)
    return ref, segs


def frame(rng, H, payload, l3=None, frag=0, ihl=5):
    fr = bytearray(rng.integers(0, 256, H + payload, np.uint8).tobytes())
    if l3 is not None:
        fr[l3] = 0x40 | ihl
        fr[l3 + 6:l3 + 8] = frag.to_bytes(2, "big")
    return bytes(fr)


FIELD = dict(mod_op=ADD, size=2, offset=16)
CHECK = [(dict(proto=IPV4), 0), (dict(proto=CUSTOM, num_custom=0), 0), (dict(proto=0), -22),
         (dict(proto=3), -22), (dict(proto=CUSTOM, num_custom=9), -22),
         *[(dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, size=s)), 0) for s in (1, 2, 4, 8)],
         *[(dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, size=s)), -22) for s in (0, 3, 16)],
         (dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, offset=128)), 0),
         (dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, offset=129)), -22),
         (dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, mod_op=2)), -22),
         (dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, mod_op=BITS, size=1)), 0),
         (dict(proto=CUSTOM, num_custom=1, f=dict(FIELD, mod_op=BITS, size=2)), -22),
         (dict(proto=IPV4, num_custom=9), 0)]   # the custom part is not read for IPv4


@pytest.mark.parametrize("case,rc", CHECK)
def test_profile_check(case, rc):
    """odp_lso_profile_create's accept / reject table; host only."""
    p = L.odpg_lso_profile_t(proto=case["proto"], num_custom=case.get("num_custom", 0))
    p.field[0] = L.odpg_lso_field_t(**case.get("f", {}))
    assert L.lib.odpg_lso_profile_check(C.byref(p)) == rc
    assert L.lib.odpg_lso_profile_check(None) == -22
    assert C.sizeof(L.odpg_lso_opt_t) == 8 and T == 64


@pytest.mark.gpu
@pytest.mark.parametrize("num", [1, 63, T + 1, 3 * T + 17])
@pytest.mark.parametrize("H", [14, 34, 54, 128])
def test_shapes(gpu_ctx, H, num):
    """Every P with payloads of m P, m P + 1 and m P + P - 1 bytes in one batch,
    both profiles alternating; 64 segments, 65 (TOO_MANY), payload == P and
    H + P > len at the end of the batch."""
    rng = np.random.default_rng(100 * H + num)
    pkts, rows = [], []
    for i in range(num):
        P = (8, 9, 100, 552, 1460)[i % 5]
        m = int(rng.integers(1, 6))
        pay = m * P + (0, 1, P - 1)[(i // 5) % 3]
        ip = H >= 34 and i % 2
        pkts.append(frame(rng, H, pay, l3=H - 20 if ip else None))
        rows.append((H, P, H - 20 if ip else NO_L3, int(ip)))
    for i, (pay, P) in enumerate([(512, 8), (513, 8), (100, 100), (99, 100)][:num]):
        pkts[-1 - i], rows[-1 - i] = frame(rng, H, pay), (H, P, NO_L3, 0)
    ref, _ = run_and_check(gpu_ctx, PROFILES, pkts, rows)
    assert ref[3][-1] == 0 and (num < 2 or ref[3][-2] == L.LSO_TOO_MANY)


@pytest.mark.gpu
@pytest.mark.parametrize("length,P,prof,n", [(325, 700, 1, 1), (1500, 1000, 1, 2),
                                             (1500, 700, 1, 3), (723, 800, 0, 1),
                                             (723, 500, 0, 2), (723, 288, 0, 3)])
@pytest.mark.parametrize("uniform", [False, True])
def test_reference_pairs(gpu_ctx, length, P, prof, n, uniform):
    """The shape pairs of test/validation/api/pktio/lso.c:1141-1152, each with
    per-packet options and with the uniform form."""
    rng = np.random.default_rng(length + P)
    H, l3 = (34, 14) if prof else (22, NO_L3)
    pkts = [frame(rng, H, length - H, l3=14 if prof else None) for _ in range(3)]
    ref, _ = run_and_check(gpu_ctx, PROFILES, pkts, [(H, P, l3, prof)] * 3, uniform=uniform)
    assert ref[4]["num_segs"] == 3 * n


@pytest.mark.gpu
@pytest.mark.parametrize("frag", [0, 0x4000, 0x2000, 100, 0x1FF0, 0xFFFF])
def test_ipv4_fragments(gpu_ctx, frag):
    """Original frag_offset 0, DF, MF, an offset, and two that wrap 16 bits.
    Independently of segment(): every header sums to 0xFFFF and the payloads
    of a packet's segments concatenate to its payload."""
    rng = np.random.default_rng(frag)
    pkts = [frame(rng, 34, pay, l3=14, frag=frag) for pay in (3000, 1473, 552 * 3, 8 * 64)]
    rows = [(34, 552, 14, 1)] * 3 + [(34, 8, 14, 1)]
    ref, segs = run_and_check(gpu_ctx, PROFILES, pkts, rows)
    first = ref[2]
    for i, p in enumerate(pkts):
        mine = segs[first[i]:first[i + 1]]
        assert len(mine) > 1 and b"".join(s[34:] for s in mine) == p[34:]
        for s in mine:
            c = sum(int.from_bytes(s[14 + j:16 + j], "big") for j in range(0, 20, 2))
            assert c % 0xFFFF == 0 and c


BITS3 = ((0xF0, 0xA0), (0x0F, 0x05), (0xFF, 0x3C))
CUSTOM_CASES = {
    "sizes": [(ADD, 2, 1), (ADD, 4, 2), (ADD, 8, 4), (ADD, 16, 8)],        # frames all 0xFF
    "bits": [(BITS, 3, 1, *BITS3), (BITS, 40, 1, *BITS3)],
    "payload": [(ADD, 60, 4), (BITS, 128, 1, *BITS3), (ADD, 128, 8)],      # beyond H = 54
    "straddle": [(ADD, 51, 8), (ADD, 53, 2)],                              # across H = 54
    "overlap": [(ADD, 10, 4), (BITS, 12, 1, *BITS3), (ADD, 11, 2), (ADD, 8, 8)],
    "none": [],
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CUSTOM_CASES)
def test_custom_fields(gpu_ctx, case):
    """Carries across every byte, WRITE_BITS on 2, 3 and more segments, fields
    in the payload, across H and overlapping (profile order matters). The
    last segments of the 316- and 82-byte payloads are 70 and 72 bytes: a
    field at 128 fails them with BAD_FIELD while the others succeed."""
    rng = np.random.default_rng(7)
    pays = (200, 300, 1000, 316, 82) * 3
    pkts = [b"\xff" * (54 + p) if case == "sizes" else frame(rng, 54, p) for p in pays]
    rows = [(54, 100 if p != 82 else 64, NO_L3, 0) for p in pays]
    ref, _ = run_and_check(gpu_ctx, [(CUSTOM, CUSTOM_CASES[case])], pkts, rows)
    short = np.isin(pays, (316, 82)) & (case == "payload")
    assert np.all(ref[3][short] == L.LSO_BAD_FIELD) and not np.any(ref[3][~short])


def failing(rng):
    """(frame, option row, status) of every reason a packet fails for."""
    def ip(**kw):
        return frame(rng, 34, 1000, l3=14, **kw)

    return [(ip(), (34, 552, 14, 2), L.LSO_BAD_PROFILE), (ip(), (129, 552, 14, 1), L.LSO_BAD_OFFSET),
            (frame(rng, 20, 0), (21, 8, NO_L3, 0), L.LSO_BAD_OFFSET),
            (ip(), (34, 552, NO_L3, 1), L.LSO_BAD_L3), (ip(), (34, 552, 35, 1), L.LSO_BAD_L3),
            (ip(), (34, 552, 15, 1), L.LSO_BAD_L3), (ip(), (34, 7, 14, 1), L.LSO_BAD_PAYLOAD),
            (ip(), (34, 0, NO_L3, 0), L.LSO_BAD_PAYLOAD), (ip(ihl=6), (34, 552, 14, 1), L.LSO_BAD_IHL),
            (ip(ihl=4), (34, 552, 14, 1), L.LSO_BAD_IHL), (ip(), (34, 15, NO_L3, 0), L.LSO_TOO_MANY)]


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["first", "middle", "nowhere"])
def test_options_and_failures(gpu_ctx, where):
    """A per-packet option array mixing both profiles and every failure;
    first_bad and seg_first with failures at index 0, in the middle, nowhere.
    An IPv4 packet with a bad IHL or L3 offset that needs no segmentation is
    sent unchanged (rule 3 comes first)."""
    rng = np.random.default_rng(11)
    good = [(frame(rng, 34, 1500, l3=14), (34, 552, 14, i % 2), 0) for i in range(T + 5)]
    good += [(frame(rng, 34, 100, l3=14, ihl=6), (34, 552, NO_L3, 1), 0)]
    bad = failing(rng)
    cases = {"first": bad + good, "middle": good[:40] + bad + good[40:], "nowhere": good}[where]
    ref, _ = run_and_check(gpu_ctx, PROFILES, [c[0] for c in cases], [c[1] for c in cases])
    assert list(ref[3]) == [c[2] for c in cases]
    assert ref[4]["first_bad"] == {"first": 0, "middle": 40, "nowhere": len(cases)}[where]


@pytest.mark.gpu
@pytest.mark.parametrize("source", ["stride", "imix"])
def test_sources(gpu_ctx, source):
    """A fixed-stride source and the IMIX length mix through descriptors,
    uniform options."""
    num = 2 * T + 3
    if source == "stride":
        pkts = [bytes(r) for r in gen.c2_frames(num * 10, seed=5).reshape(num, 640)]
        run_and_check(gpu_ctx, PROFILES, pkts, [(34, 96, 14, 1)] * num, uniform=True, stride=640)
    else:
        frames, desc = gen.c3_frames(num, seed=5)
        pkts = [bytes(frames[d["offset"]:d["offset"] + d["len"]]) for d in desc]
        ref, _ = run_and_check(gpu_ctx, PROFILES, pkts, [(34, 552, NO_L3, 0)] * num, uniform=True)
        assert ref[4]["num_segs"] > num


@pytest.mark.gpu
@pytest.mark.parametrize("cut", ["bytes", "segs", "zero"])
def test_capacity(gpu_ctx, cut):
    """A byte capacity that ends inside a packet's segments, max_segs that cuts
    first, and both zero: the copied prefix, {0, 0} descriptors, the fill
    beyond, total.bytes and num_segs still the full need."""
    rng = np.random.default_rng(13)
    num = T + 9
    pkts = [frame(rng, 54, 2000 + i) for i in range(num)]       # 4 segments each
    rows = [(54, 552, NO_L3, 0)] * num
    per = [3 * 608 + (54 + 2000 + i - 3 * 552 + 15) // 16 * 16 for i in range(num)]
    cap, max_segs = {"bytes": (sum(per[:T + 2]) + 2 * 608 + 100, 4 * num),
                     "segs": (sum(per), 4 * (T + 1) + 2), "zero": (0, 0)}[cut]
    ref, _ = run_and_check(gpu_ctx, PROFILES, pkts, rows, cap=cap, max_segs=max_segs)
    tot = ref[4]
    assert tot["bytes"] == sum(per) and tot["num_segs"] == 4 * num
    assert tot["copied"] == {"bytes": 4 * (T + 2) + 2, "segs": max_segs, "zero": 0}[cut]


@pytest.mark.gpu
def test_arguments(gpu_ctx):
    """Every -EINVAL of the header returns before a launch: the outputs still
    hold their fill after a sync. Create refuses bad profile sets."""
    bad = L.lso_profile(CUSTOM, [(BITS, 0, 2)])
    h = C.c_void_p()
    for profs in ([], [bad], [L.lso_profile(IPV4)] * 17):
        arr = (L.odpg_lso_profile_t * max(len(profs), 1))(*profs)
        assert L.lib.odpg_lso_create(gpu_ctx.h, arr, len(profs), 8, C.byref(h)) == -22
    plan = gpu_ctx.lso([L.lso_profile(IPV4)], 100)
    fb, db, ob, gb, sb, tb = (gpu_ctx.buffer(6400) for _ in range(6))
    for b in (gb, sb, tb):
        b.upload(np.full(1600, 0xA5A5A5A5, np.uint32))
    good_s = dict(frames=fb.ptr, desc=db.ptr, stride=0, num=100, opt=ob.ptr)
    good_d = dict(frames=gb.ptr, capacity=6400, desc=gb.ptr, max_segs=10, seg_first=sb.ptr,
                  status=sb.ptr, total=tb.ptr)
    cases = [(dict(num=101), {}), (dict(frames=None), {}), (dict(frames=fb.ptr + 8), {}),
             (dict(desc=None, stride=0), {}), (dict(desc=None, stride=72), {}),
             ({}, dict(frames=None)), ({}, dict(frames=gb.ptr + 4)), ({}, dict(desc=None)),
             ({}, dict(seg_first=None)), ({}, dict(status=None)), ({}, dict(total=None)),
             ({}, dict(capacity=(1 << 32) + 1))]
    for ds, dd in cases:
        s, d = L.odpg_lso_src_t(**{**good_s, **ds}), L.odpg_lso_dst_t(**{**good_d, **dd})
        assert L.lib.odpg_lso(plan.h, C.byref(s), C.byref(d)) == -22, (ds, dd)
    s, d = L.odpg_lso_src_t(**good_s), L.odpg_lso_dst_t(**good_d)
    assert L.lib.odpg_lso(None, C.byref(s), C.byref(d)) == -22
    assert L.lib.odpg_lso(plan.h, None, C.byref(d)) == L.lib.odpg_lso(plan.h, C.byref(s), None) == -22
    gpu_ctx.sync()
    for b in (gb, sb, tb):
        assert np.all(b.download(np.uint32, 1600) == 0xA5A5A5A5)
    # an empty batch writes seg_first[0] and total only
    s.num = 0
    assert L.lib.odpg_lso(plan.h, C.byref(s), C.byref(d)) == 0
    gpu_ctx.sync()
    assert tb.download(TOTAL_DT, 1)[0].tolist() == (0, 0, 0, 0, 0)
    assert sb.download(np.uint32, 2).tolist() == [0, 0xA5A5A5A5]
    assert np.all(gb.download(np.uint32, 1600) == 0xA5A5A5A5)
    plan.close()


@pytest.mark.gpu
def test_pipeline_without_sync(gpu_ctx, fresh_cls):
    """odpg_lso then odpg_classify of its output on the same stream, one sync
    at the end: verdicts and odpg_meta_t equal the oracle's on the restated
    segments; every fragment has L3 checksum OK and the ipfrag flag."""
    num, opt = T + 7, L.PKTIN_IPV4_CHKSUM
    p = fresh_cls.loop_pktio(pktin=opt)
    gen.build_c2_rules(fresh_cls, p)
    assert fresh_cls.pktio_start(p) == 0
    rules = fresh_cls.pktio_rules(p)
    tbl = gpu_ctx.table(rules)
    pkts = [bytes(r) for r in gen.c2_frames(num * 25, seed=3).reshape(num, 1600)]
    opts = opt_array([(34, 552, 14, 1)] * num)
    cap = num * 3 * 592
    ref, segs = expected(pkts, opts, PROFILES, cap, 3 * num)
    n2 = len(segs)
    assert n2 == 3 * num == ref[4]["copied"]
    meta_dt = L.np_dtypes()[0]
    plan = gpu_ctx.lso([L.lso_profile(*q) for q in PROFILES], num)
    bufs = [gpu_ctx.buffer(n) for n in (1600 * num + 64, 8 * num, cap + 64, 8 * n2, 4 * num + 4,
                                        num, 24, 4 * n2, meta_dt.itemsize * n2)]
    fb, ob, gfb, gdb, sb, stb, tb, vb, mb = bufs
    fb.upload(np.frombuffer(b"".join(pkts), np.uint8))
    ob.upload(opts)
    plan.run_dev(fb, num, gfb, cap, gdb, n2, sb, stb, tb, stride=1600, opt_buf=ob)
    gpu_ctx.classify_dev(tbl, gfb, n2, desc_buf=gdb, opt=opt, out_buf=vb, meta_buf=mb)
    gpu_ctx.sync()
    o = oracle.classify(rules, ref[0], n2, desc=ref[1], opt=opt)
    meta = mb.download(meta_dt, n2)
    assert np.array_equal(vb.download(np.uint32, n2), o["out"])
    assert meta.tobytes() == o["meta"].tobytes()
    assert all(has(m, "ipfrag") for m in meta) and np.all(L.out_l3(o["out"]) == L.ODPG_CHKSUM_OK)
    for b in bufs:
        b.free()
    plan.close()
