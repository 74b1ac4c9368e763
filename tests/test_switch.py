"""L2 learning-switch forwarding of a device-resident batch (include/odpg_switch.h).

Reference: reference() below, the header's sequential loop over a list of
65536 integers, with a bitwise CRC32C. Everything is compared exactly: out,
every port's list and count, total and the whole table. Output buffers are
prefilled with 0xA5, so a stray write shows, list words at and beyond
count[p] included.

A batch is a named scenario, then traffic among the same few hosts up to the
size (so one slot's writer run spans several tiles). A scenario's frames
carry the out word its name promises; those depend on earlier frames only, so
they hold for every prefix the sizes cut. T = the packets one workgroup of the
resolve and list kernels handles."""
import ctypes as C
import itertools

import numpy as np
import pytest

import oracle
from odp_amd import _lib as L

T = L.SWITCH_TILE
_, DESC_DT = L.np_dtypes()
TOTAL_DT = np.dtype(L.SWITCH_TOTAL_FIELDS)
SIZES = [1, T - 1, T, T + 1, 4 * T + 3]
FILL32 = 0xA5A5A5A5
FL, DF, DP = L.SWITCH_FLOOD << 8, L.SWITCH_DROP_FRAME << 8, L.SWITCH_DROP_PORT << 8
BC, Z = b"\xff" * 6, bytes(6)
A, B, D, E, F = (bytes([2, 0, 0, 0, 0, k]) for k in range(1, 6))
X, Y = bytes.fromhex("020000000d90"), bytes.fromhex("020000004000")   # one slot, 0x66C7
M = bytes.fromhex("02000000b5bf")                                      # slot 0xFFFF
HOME = {A: 1, B: 2, D: 3, E: 4, F: 5, X: 6, Y: 7, M: 0}               # a host's port
LENS = [60, 14, 15, 1514]


def crc32c(data):
    c = 0
    for x in data:
        c ^= x
        for _ in range(8):
            c = (c >> 1) ^ (0x82F63B78 if c & 1 else 0)
    return c


def slot(mac):
    return crc32c(mac) & 0xFFFF


def entry(mac, port, tick):
    return int.from_bytes(mac + bytes([port, tick]), "little")


def reference(pkts, ports, P, tick, table):
    """(out, the ports' lists) of the batch; table, 65536 integers, is updated."""
    out, lists = [], [[] for _ in range(P)]
    for i, (fr, p) in enumerate(zip(pkts, ports)):
        dst, src = fr[:6], fr[6:12]
        if len(fr) < 14 or (p < P and (src in (BC, Z) or dst == Z)):
            out.append(DF)
            continue
        if p >= P:
            out.append(DP)
            continue
        table[slot(src)] = entry(src, p, tick)
        e = table[slot(dst)].to_bytes(8, "little")
        diff = tick - e[7] if e[7] < tick else (255 + tick - e[7]) & 255 if e[7] > tick else 0
        if dst != BC and e[:6] == dst and diff <= L.SWITCH_AGING_TIME:
            out.append(e[6])
            lists[e[6]] += [i] if e[6] < P else []
        else:
            out.append(FL)
            for q in range(P):
                lists[q] += [i] if q != p else []
    return out, lists


# a scenario: (frames as (dst, src, port_in, out word, length or None), tick, preloaded entries)
def s_learn():       # learned earlier: UNICAST; learned only later: FLOOD
    return [(B, A, 1, FL), (A, B, 2, 1), (B, A, 1, 2)], 0, []


def s_self():
    return [(A, A, 1, 1)], 0, []


def s_collide():     # X and Y alternate as the owners of one slot
    return [(BC, X, 6, FL), (X, B, 2, 6), (Y, B, 2, FL), (BC, Y, 7, FL), (Y, B, 2, 7), (X, B, 2, FL),
            (BC, X, 6, FL), (X, B, 2, 6), (Y, B, 2, FL)], 0, []


def s_last_slot():
    return [(BC, M, 0, FL), (M, A, 1, 0)], 0, []


def s_move():
    return [(BC, A, 1, FL), (A, B, 2, 1), (BC, A, 5, FL), (A, B, 2, 5)], 0, []


def s_invalid():     # none of them learns D
    return [(A, BC, 1, DF), (A, Z, 1, DF), (Z, D, 3, DF), (B, D, 3, DF, 13), (B, D, 200, DP),
            (D, A, 1, FL)], 0, []


def s_bcast_learns():
    return [(BC, A, 1, FL), (A, B, 2, 1)], 0, []


def s_aging():       # tick distances 0, 5 and 6
    return [(A, F, 5, 1), (B, F, 5, 2), (D, F, 5, FL)], 10, [(A, 1, 10), (B, 2, 5), (D, 3, 4)]


def s_aging_wrap():  # 2 against 252: 5; against 251: 6; equal; an entry from the future: 254
    return ([(A, F, 5, 1), (B, F, 5, FL), (D, F, 5, 3), (E, F, 5, FL)], 2,
            [(A, 1, 252), (B, 2, 251), (D, 3, 2), (E, 4, 3)])


SCENARIOS = {f.__name__[2:]: f for f in (s_learn, s_self, s_collide, s_last_slot, s_move, s_invalid,
                                         s_bcast_learns, s_aging, s_aging_wrap)}
assert oracle.crc32c(A, 0) == crc32c(A) and slot(X) == slot(Y) == 0x66C7 and slot(M) == 0xFFFF


def batch(items, size, seed, P=8, uniform=None, stride=0):
    """(frames, ports, wants): the scenario's frames, then traffic among the hosts."""
    rng = np.random.default_rng(seed)
    hosts = list(HOME)
    while len(items) < size:
        d, s = rng.choice(len(hosts), 2)
        items = items + [(hosts[d] if rng.random() < 0.9 else BC, hosts[s], HOME[hosts[s]], None)]
    pkts, ports = [], []
    for i, (dst, src, port, _, *ln) in enumerate(items[:size]):
        n = stride or (ln[0] if ln else LENS[i % 4])
        pkts.append((dst + src + rng.bytes(1502))[:n])
        ports.append((port if port >= 32 else port % P) if uniform is None else uniform)
    return pkts, ports, [w for _, _, _, w, *_ in items[:size]]


def run_and_check(plan, pkts, ports, tick, table, stride=0):
    """Switch on the GPU and compare every output and the table; returns the reference's out."""
    P, num, ls = plan.num_ports, len(pkts), len(pkts) + 3
    out, lists = reference(pkts, ports, P, tick, table)
    if stride:
        buf, desc = np.frombuffer(b"".join(pkts), np.uint8), None
    else:
        desc = np.zeros(num, DESC_DT)
        desc["len"] = [len(p) for p in pkts]
        al = (desc["len"].astype(np.int64) + 15) // 16 * 16
        desc["offset"] = np.cumsum(al) - al
        buf = np.random.default_rng(1).integers(0, 256, int(al.sum()) + 64, np.uint8)
        for p, d in zip(pkts, desc):
            buf[d["offset"]:d["offset"] + d["len"]] = np.frombuffer(p, np.uint8)
    uniform = len(set(ports)) == 1
    got = plan.run(buf, ports[0] if uniform else ports, tick, stride=stride, desc=desc,
                   list_stride=ls, fill=0xA5)
    want_lists = np.full((P, ls), FILL32, np.uint32)
    for p, l in enumerate(lists):
        want_lists[p, :len(l)] = l
    kinds = np.array(out) >> 8
    ref = (np.array(out, np.uint32), want_lists,
           np.array([[0, len(l)] for l in lists], np.uint32).ravel(),
           np.array((np.count_nonzero(kinds == 0), np.count_nonzero(kinds == 1),
                     np.count_nonzero(kinds >= 2), sum(map(len, lists))), TOTAL_DT),
           np.array(table, "<u8"))
    for name, g, r in zip(("out", "lists", "port_offsets", "total", "table"), (*got, plan.table()), ref):
        assert np.asarray(g).tobytes() == r.tobytes(), (name, g, r)
    return out, got


def fresh(ctx, P, num, preload=()):
    plan, table = ctx.switch(P, num), [0] * L.SWITCH_TABLE_SIZE
    for mac, port, tick in preload:
        table[slot(mac)] = entry(mac, port, tick)
    if preload:
        plan.set_table(table)
    return plan, table


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("name", SCENARIOS)
def test_scenarios(gpu_ctx, name, size):
    """8 ports, a port per packet, descriptors with lengths 13, 14, 15, 60 and 1514."""
    items, tick, preload = SCENARIOS[name]()
    pkts, ports, wants = batch(items, size, 1000 * sorted(SCENARIOS).index(name) + size)
    plan, table = fresh(gpu_ctx, 8, size, preload)
    out, _ = run_and_check(plan, pkts, ports, tick, table)
    plan.close()
    k = min(size, len(items))
    assert out[:k] == wants[:k]           # the scenario did what its name says


MIXED = [it for f in (s_collide, s_move, s_invalid, s_last_slot, s_self) for it in f()[0]]


@pytest.mark.gpu
@pytest.mark.parametrize("P,uniform,stride", itertools.product([2, 8, 32], [None, 1], [0, 64]))
def test_shapes(gpu_ctx, P, uniform, stride):
    """2, 8 and 32 ports; a port per packet and one for all; descriptors and a fixed stride."""
    pkts, ports, _ = batch(MIXED, SIZES[-1], P, P, uniform, stride)
    plan, table = fresh(gpu_ctx, P, len(pkts))
    run_and_check(plan, pkts, ports, 7, table, stride)
    plan.close()


@pytest.mark.gpu
def test_partition_tiles(gpu_ctx):
    """More than two tiles of the radix partition, one slot's writers in all of them."""
    pkts, ports, _ = batch(s_collide()[0], 2 * L.DELIVER_TILE + 5, 5, stride=64)
    plan, table = fresh(gpu_ctx, 8, len(pkts))
    run_and_check(plan, pkts, ports, 0, table, 64)
    plan.close()


@pytest.mark.gpu
def test_second_call_relies_on_first(gpu_ctx):
    """The table carries from call to call: learned at tick 3, hit at tick 8."""
    plan, table = fresh(gpu_ctx, 8, T)
    pkts, ports, _ = batch([(BC, A, 1, FL)], 1, 0)
    assert run_and_check(plan, pkts, ports, 3, table)[0] == [FL]
    pkts, ports, _ = batch([(A, B, 2, 1)], T, 1)
    assert run_and_check(plan, pkts, ports, 8, table)[0][0] == 1
    plan.close()


@pytest.mark.gpu
def test_flood_list_feeds_gather(gpu_ctx):
    """Port 1's list of a flooding batch is a one-bucket delivery list: odpg_gather of it
    yields those frames in list order."""
    pkts, ports, _ = batch([(BC, A, 2, FL)] * 5 + s_move()[0], T + 9, 3, stride=64)
    plan, table = fresh(gpu_ctx, 8, len(pkts))
    _, got = run_and_check(plan, pkts, ports, 0, table, 64)
    plan.close()
    cnt = int(got[2][3])
    g = gpu_ctx.gather(len(pkts))
    frames, gdesc, _, total = g.run(np.frombuffer(b"".join(pkts), np.uint8), got[1][1][:len(pkts)],
                                    got[2][2:4], 0, 1, stride=64)
    g.close()
    assert total["num"] == total["copied"] == cnt > 5
    assert [bytes(frames[d["offset"]:d["offset"] + d["len"]]) for d in gdesc[:cnt]] == \
        [pkts[i] for i in got[1][1][:cnt]]


BAD_ARGS = [(dict(num=101), {}), (dict(frames=None), {}), (dict(frames=8), {}),
            (dict(desc=None, stride=0), {}), (dict(desc=None, stride=72), {}), ({}, dict(out=None)),
            ({}, dict(lists=None)), ({}, dict(port_offsets=None)), ({}, dict(total=None)),
            ({}, dict(list_stride=99)), "plan", "src", "dst"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAD_ARGS, ids=str)
def test_arguments(gpu_ctx, case):
    """Every -EINVAL of the header returns before a launch: the outputs still
    hold their fill after a sync. An int stands for that offset into the frames.
    An empty batch writes total and port_offsets only."""
    plan = gpu_ctx.switch(4, 100)
    fb, ob = gpu_ctx.buffer(6400), gpu_ctx.buffer(4096)
    ob.upload(np.full(1024, FILL32, np.uint32))
    good_s = dict(frames=fb.ptr, desc=fb.ptr, stride=0, num=100, port_in=fb.ptr)
    good_d = dict(out=ob.ptr, lists=ob.ptr + 512, list_stride=100, port_offsets=ob.ptr + 3072,
                  total=ob.ptr + 3200)
    ds, dd = case if isinstance(case, tuple) else ({}, {})
    if ds.get("frames"):
        ds = dict(ds, frames=fb.ptr + ds["frames"])
    s, d = L.odpg_switch_src_t(**{**good_s, **ds}), L.odpg_switch_dst_t(**{**good_d, **dd})
    args = [None if case == "plan" else plan.h, None if case == "src" else C.byref(s), 0,
            None if case == "dst" else C.byref(d)]
    assert L.lib.odpg_switch(*args) == -22
    h = C.c_void_p()
    for ports, pk in ((1, 100), (33, 100), (4, (1 << 24) + 1)):
        assert L.lib.odpg_switch_create(gpu_ctx.h, ports, pk, C.byref(h)) == -22
    gpu_ctx.sync()
    assert np.all(ob.download(np.uint32, 1024) == FILL32)
    s = L.odpg_switch_src_t(**{**good_s, "num": 0})
    assert L.lib.odpg_switch(plan.h, C.byref(s), 0, C.byref(L.odpg_switch_dst_t(**good_d))) == 0
    gpu_ctx.sync()
    after = ob.download(np.uint32, 1024)
    assert after[768:776].tolist() == [0] * 8 and after[800:804].tolist() == [0] * 4
    after[768:776] = after[800:804] = FILL32
    assert np.all(after == FILL32)
    plan.close()
    fb.free()
    ob.free()
