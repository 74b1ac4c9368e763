"""odpg_esp (include/odpg_esp.h) against a plain reference: AES, GCM with a
bitwise GF(2^128) multiply and the header's packet rules as a sequential loop
over Python integers and bytes. Everything is compared byte for byte: frames
(the whole destination buffer, prefilled with 0xA5), desc, status, seq, total
and next_seq."""
import ctypes as C
import itertools
import struct

import numpy as np
import pytest

from odp_amd import _lib as L

T = L.ESP_TILE
FILL = 0xA5
DESC_DT = np.dtype([("offset", "<u4"), ("len", "<u4")])
TOTAL_DT = np.dtype(L.ESP_TOTAL_FIELDS)
LENGTHS = [20, 21, 22, 23, 30, 34, 46, 1006, 1007, 1022, 1023, 1024, 1038, 1039, 1500]


# ---- reference: AES, GCM ------------------------------------------------------
def _sbox():
    s, p, q = [0x63] * 256, 1, 1
    rol = lambda v, n: ((v << n) | (v >> (8 - n))) & 0xFF
    while True:
        p = (p ^ (p << 1) ^ (0x1B if p & 0x80 else 0)) & 0xFF
        q ^= (q << 1) & 0xFF
        q ^= (q << 2) & 0xFF
        q ^= (q << 4) & 0xFF
        q ^= 0x09 if q & 0x80 else 0
        s[p] = q ^ rol(q, 1) ^ rol(q, 2) ^ rol(q, 3) ^ rol(q, 4) ^ 0x63
        if p == 1:
            return s


SBOX = _sbox()
xt = lambda b: ((b << 1) ^ (0x1B if b & 0x80 else 0)) & 0xFF


def expand(key):
    """FIPS-197 5.2: the round keys as 4 (Nr + 1) big-endian words."""
    nk = len(key) // 4
    w = list(struct.unpack(f">{nk}I", key))
    rcon = 1
    sub = lambda v: int.from_bytes(bytes(SBOX[b] for b in v.to_bytes(4, "big")), "big")
    for i in range(nk, 4 * (nk + 7)):
        t = w[-1]
        if i % nk == 0:
            t = sub(((t << 8) | (t >> 24)) & 0xFFFFFFFF) ^ (rcon << 24)
            rcon = xt(rcon)
        elif nk > 6 and i % nk == 4:
            t = sub(t)
        w.append(w[i - nk] ^ t)
    return w


def aes(w, block):
    rk = [struct.pack(">4I", *w[i:i + 4]) for i in range(0, len(w), 4)]
    s = bytes(a ^ b for a, b in zip(block, rk[0]))
    for r in range(1, len(rk)):
        s = bytes(SBOX[s[(i + 4 * (i % 4)) % 16]] for i in range(16))   # SubBytes, ShiftRows
        if r < len(rk) - 1:
            m = bytearray()
            for c in range(0, 16, 4):
                a = s[c:c + 4]
                x = a[0] ^ a[1] ^ a[2] ^ a[3]
                m += bytes(a[i] ^ x ^ xt(a[i] ^ a[(i + 1) % 4]) for i in range(4))
            s = bytes(m)
        s = bytes(a ^ b for a, b in zip(s, rk[r]))
    return s


def gmul(x, y):
    z = 0
    for i in range(127, -1, -1):
        if (x >> i) & 1:
            z ^= y
        y = (y >> 1) ^ (0xE1 << 120 if y & 1 else 0)
    return z


def gcm(key, nonce, aad, data):
    """(data XOR keystream, tag function): tag(ct) is the ICV for ciphertext ct."""
    w = expand(key)
    h = int.from_bytes(aes(w, bytes(16)), "big")
    ks = b"".join(aes(w, nonce + struct.pack(">I", 2 + i)) for i in range((len(data) + 15) // 16))
    out = bytes(a ^ b for a, b in zip(data, ks))

    def tag(ct):
        y = 0
        for part in (aad, ct):
            for i in range(0, len(part), 16):
                y = gmul(y ^ int.from_bytes(part[i:i + 16].ljust(16, b"\0"), "big"), h)
        y = gmul(y ^ (len(aad) * 8 << 64 | len(ct) * 8), h)
        return bytes(a ^ b for a, b in zip(y.to_bytes(16, "big"), aes(w, nonce + b"\0\0\0\1")))
    return out, tag


# FIPS-197 C.1 and test case 4 of the GCM specification
assert aes(expand(bytes(range(16))), bytes.fromhex("00112233445566778899aabbccddeeff")).hex() == \
    "69c4e0d86a7b0430d8cdb78070b4c55a"
_c, _t = gcm(bytes.fromhex("feffe9928665731c6d6a8f9467308308"), bytes.fromhex("cafebabefacedbaddecaf888"),
             bytes.fromhex("feedfacedeadbeeffeedfacedeadbeefabaddad2"),
             bytes.fromhex("d9313225f88406e5a55909c5aff5269a86a7a9531534f7da2e4c303d8a318a72"
                           "1c3c0c95956809532fcf0e2449a6b525b16aedf5aa0de657ba637b39"))
assert _c.hex().startswith("42831ec221777424") and _t(_c).hex() == "5bc94fbc3221a5db94fae95ae7121a47"


# ---- reference: the packet rules ----------------------------------------------
def sa_of(k, key_len=16, **kw):
    rng = np.random.default_rng(77 + k)
    return dict(dict(spi=0x1000 + k, key=rng.bytes(key_len), salt=rng.bytes(4), tun_src=rng.bytes(4),
                     tun_dst=rng.bytes(4), ttl=64 - k, dscp=0, df=0, copy_dscp=0, copy_df=0,
                     mtu=0xFFFF), **kw)


def csum(h):
    s = sum(struct.unpack(f">{len(h) // 2}H", h))
    s = (s & 0xFFFF) + (s >> 16)
    return ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF


def encap(pre, pt, sa, seq64, tos=0, df=0, opts=b"", crypt=True):
    """pre | outer IPv4 (with options `opts`) | ESP | IV | ciphertext | ICV; pt holds the
    trailer. crypt=False: the frame's length only, plaintext in place of ciphertext."""
    frag = 0x4000 if df else 0
    ip = struct.pack(">BBHHHBBH", 0x45 + len(opts) // 4, tos, 52 + len(opts) + len(pt),
                     0 if frag else seq64 & 0xFFFF, frag, sa["ttl"], 50, 0) + sa["tun_src"] + sa["tun_dst"] + opts
    ip = ip[:10] + struct.pack(">H", csum(ip)) + ip[12:]
    esp, iv = struct.pack(">II", sa["spi"], seq64 & 0xFFFFFFFF), struct.pack("<Q", seq64)
    ct, tag = gcm(sa["key"], sa["salt"] + iv, esp, pt) if crypt else (pt, lambda ct: bytes(16))
    return pre + ip + esp + iv + ct + tag(ct)


def trailer(inner, nxt):
    p = -(len(inner) + 2) % 4
    return inner + bytes(range(1, p + 1)) + bytes([p, nxt])


def ref_out(fr, Lo, sa, seq64, crypt=True):
    """(status, frame) of one outbound packet; seq64 is the number it would take."""
    n = len(fr)
    if sa is None:
        return L.ESP_NO_SA, None
    if Lo + 20 > n:
        return L.ESP_BAD_L3, None
    ver = fr[Lo] >> 4
    if ver == 4 and fr[Lo] & 15 >= 5 and (fr[Lo + 2] << 8 | fr[Lo + 3]) >= 4 * (fr[Lo] & 15):
        ip_len, nxt, tos, df = fr[Lo + 2] << 8 | fr[Lo + 3], 4, fr[Lo + 1], fr[Lo + 6] & 0x40
    elif ver == 6 and Lo + 40 <= n:
        ip_len, nxt, df = 40 + (fr[Lo + 4] << 8 | fr[Lo + 5]), 41, 0
        tos = (fr[Lo] & 15) << 4 | fr[Lo + 1] >> 4
    else:
        return L.ESP_BAD_L3, None
    if Lo + ip_len > n:
        return L.ESP_BAD_L3, None
    if 52 + ((ip_len + 5) & ~3) > sa["mtu"]:
        return L.ESP_MTU, None
    return L.ESP_OK, encap(fr[:Lo], trailer(fr[Lo:Lo + ip_len], nxt), sa, seq64,
                           tos if sa["copy_dscp"] else (tos & 3) | sa["dscp"] << 2,
                           df if sa["copy_df"] else sa["df"], crypt=crypt)


def ref_in(fr, Lo, sa):
    """(status, seq, reserved bytes, frame) of one inbound packet."""
    n = len(fr)
    if sa is None:
        return L.ESP_NO_SA, 0, 0, None
    if Lo + 20 > n:
        return L.ESP_BAD_L3, 0, 0, None
    ihl, tot = fr[Lo] & 15, fr[Lo + 2] << 8 | fr[Lo + 3]
    if fr[Lo] >> 4 != 4 or ihl < 5 or (fr[Lo + 6] << 8 | fr[Lo + 7]) & 0x3FFF or tot > n - Lo:
        return L.ESP_BAD_L3, 0, 0, None
    if fr[Lo + 9] != 50:
        return L.ESP_BAD_PROTO, 0, 0, None
    if tot < 4 * ihl + 34:
        return L.ESP_BAD_LEN, 0, 0, None
    e = Lo + 4 * ihl
    spi, seq = struct.unpack(">II", fr[e:e + 8])
    if spi != sa["spi"]:
        return L.ESP_BAD_SPI, seq, 0, None
    Cn = tot - 4 * ihl - 32
    ct, res = fr[e + 16:e + 16 + Cn], Lo + Cn - 2
    pt, tag = gcm(sa["key"], sa["salt"] + fr[e + 8:e + 16], fr[e:e + 8], ct)
    if tag(ct) != fr[e + 16 + Cn:e + 32 + Cn]:
        return L.ESP_AUTH, seq, res, None
    p, nxt = pt[-2], pt[-1]
    if p + 2 > Cn or pt[Cn - 2 - p:Cn - 2] != bytes(range(1, p + 1)):
        return L.ESP_BAD_PAD, seq, res, None
    if nxt not in (4, 41):
        return L.ESP_BAD_NEXT, seq, res, None
    return L.ESP_OK, seq, res, fr[:Lo] + pt[:Cn - 2 - p]


def reference(direction, pkts, sas, sa_idx, Ls, next_seq, only=None):
    """Per packet (status, seq, reserved, frame); advances next_seq. Outbound frames
    outside `only` are not encrypted and come back as None."""
    res = []
    for i, (fr, s, Lo) in enumerate(zip(pkts, sa_idx, Ls)):
        sa = sas[s] if s < len(sas) else None
        if direction == L.ESP_IN:
            res.append(ref_in(fr, Lo, sa))
            continue
        full = only is None or i in only
        st, out = ref_out(fr, Lo, sa, next_seq[s] if sa else 0, full)
        seq = 0
        if st == L.ESP_OK:
            seq, next_seq[s] = next_seq[s] & 0xFFFFFFFF, next_seq[s] + 1
        res.append((st, seq, len(out) if st == L.ESP_OK else 0, out if full else None))
    return res


# ---- building batches, running, comparing ---------------------------------------
def ipv4(rng, ip_len, df=0, tos=0, ihl=5):
    h = struct.pack(">BBHHHBBH", 0x40 | ihl, tos, ip_len, 7, 0x4000 if df else 0, 9, 17, 0)
    return (h + rng.bytes(4 * ihl - 12 + ip_len))[:ip_len]


def ipv6(rng, payload):
    return struct.pack(">IHBB", 0x6AB00000, payload, 17, 9) + rng.bytes(32 + payload)


def run_and_check(ctx, direction, sas, pkts, sa_idx, Ls, plan=None, next_seq=None, capacity=None,
                  max_out=None, only=None, stride=0):
    """Run the batch on the GPU and compare everything; returns (results, plan, next_seq)."""
    num = len(pkts)
    if plan is None:
        plan = ctx.esp(direction, max(len(sas), 1), max(num, 1))
        for k, sa in enumerate(sas):
            if sa:
                plan.set_sa(k, L.esp_sa(**sa))
        nxt = [1 if sa else 0 for sa in sas] or [0]
        for k, v in (next_seq or {}).items():
            nxt[k] = v
        if direction == L.ESP_OUT:
            plan.set_next_seq(nxt)
        next_seq = nxt
    res = reference(direction, pkts, sas, sa_idx, Ls, next_seq, only)
    al = np.array([(r[2] + 15) // 16 * 16 for r in res], np.int64)
    offs = np.cumsum(al) - al
    need = int(al.sum())
    capacity = need if capacity is None else need + capacity if capacity < 0 else capacity
    max_out = num if max_out is None else max_out
    want_fr = np.full(capacity + 64, FILL, np.uint8)
    want_desc = np.zeros(max_out, DESC_DT)
    copied, skip = 0, np.zeros(capacity + 64, bool)
    for i, (st, _, r, fr) in enumerate(res):
        if i < max_out and offs[i] + al[i] <= capacity:
            copied += 1
            want_desc[i] = (offs[i], len(fr) if fr is not None else r if st == L.ESP_OK else 0)
            if fr is not None:
                want_fr[offs[i]:offs[i] + len(fr)] = np.frombuffer(fr, np.uint8)
                want_fr[offs[i] + len(fr):offs[i] + (len(fr) + 15) // 16 * 16] = 0
            elif st == L.ESP_OK:
                skip[offs[i]:offs[i] + al[i]] = True
    bad = [i for i, r in enumerate(res) if r[0] != L.ESP_OK]
    want_total = np.array((num - len(bad), copied, bad[0] if bad else num, 0, need), TOTAL_DT)
    if stride:
        buf, desc = np.frombuffer(b"".join(pkts), np.uint8), None
    else:
        desc = np.zeros(num, DESC_DT)
        desc["len"] = [len(p) for p in pkts]
        sal = (desc["len"].astype(np.int64) + 15) // 16 * 16
        desc["offset"] = np.cumsum(sal) - sal
        buf = np.random.default_rng(1).integers(0, 256, int(sal.sum()) + 64, np.uint8)
        for p, d in zip(pkts, desc):
            buf[d["offset"]:d["offset"] + d["len"]] = np.frombuffer(p, np.uint8)
    uni = lambda v: v[0] if len(set(v)) == 1 else v
    got = plan.run(buf, uni(sa_idx), uni(Ls), stride=stride, desc=desc, capacity=capacity,
                   max_out=max_out, fill=FILL)
    got_fr = np.where(skip, want_fr, got[0])
    ref = (want_fr, want_desc, np.array([r[0] for r in res], np.uint8),
           np.array([r[1] for r in res], np.uint32), want_total)
    for name, g, r in zip(("frames", "desc", "status", "seq", "total"), (got_fr, *got[1:]), ref):
        assert np.asarray(g).tobytes() == r.tobytes(), (name, g, r)
    if direction == L.ESP_OUT:
        assert plan.next_seq().tolist() == next_seq
    return res, plan, next_seq


def frames_of(rng, inners, Ls, pad=True):
    """An Ethernet-like prefix of L bytes, the inner packet, on odd indices a trailing pad."""
    return [rng.bytes(Lo) + p + (rng.bytes(1 + i % 7) if pad and i & 1 else b"")
            for i, (p, Lo) in enumerate(zip(inners, Ls))]


def mixed(rng, n, nsa):
    """IMIX-like inner packets, every fifth IPv6, SAs interleaved."""
    lens = [int(rng.choice([40, 64, 576, 1500], p=[0.3, 0.3, 0.25, 0.15])) for _ in range(n)]
    inners = [ipv6(rng, ln - 40) if i % 5 == 4 else ipv4(rng, ln, df=i & 1, tos=(37 * i) & 0xFF)
              for i, ln in enumerate(lens)]
    Ls = [14 if i % 3 else 18 for i in range(n)]
    return frames_of(rng, inners, Ls), [(i * 3) % nsa for i in range(n)], Ls


SAS5 = [sa_of(0), sa_of(1, 24, copy_dscp=1), sa_of(2, 32, copy_df=1), sa_of(3, df=1, dscp=46),
        sa_of(4, 32, dscp=10, copy_df=1)]


# ---- tests ------------------------------------------------------------------------
def test_key_schedule():
    """odpg_esp_key_schedule on the host: the expansion and H for the three key lengths."""
    for n in (16, 24, 32):
        key = np.random.default_rng(n).bytes(n)
        rk, h = (C.c_uint32 * 60)(), (C.c_uint8 * 16)()
        assert L.lib.odpg_esp_key_schedule(key, n, rk, h) == 0
        w = expand(key)
        assert list(rk) == w + [0] * (60 - len(w)) and bytes(h) == aes(w, bytes(16))
    rk, h = (C.c_uint32 * 60)(), (C.c_uint8 * 16)()
    assert L.lib.odpg_esp_key_schedule(bytes(32), 20, rk, h) == -22
    for args in ((None, 16, rk, h), (bytes(16), 16, None, h), (bytes(16), 16, rk, None)):
        assert L.lib.odpg_esp_key_schedule(*args) == -22


@pytest.mark.gpu
@pytest.mark.parametrize("key_len,Lo", [*itertools.product([16, 24, 32], [14, 18]), (16, 0)])
def test_out_lengths(gpu_ctx, key_len, Lo):
    """Every pad length, the block edge and the 16-block chunk edges; a pad behind odd frames."""
    rng = np.random.default_rng(key_len + Lo)
    Ls = [Lo] * len(LENGTHS)
    pkts = frames_of(rng, [ipv4(rng, n, tos=n & 0xFF) for n in LENGTHS], Ls)
    run_and_check(gpu_ctx, L.ESP_OUT, [sa_of(0, key_len)], pkts, [0] * len(pkts), Ls)[1].close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", [1, T - 1, T, T + 1, 4 * T + 3])
def test_out_batches(gpu_ctx, size):
    """Five SAs interleaved, IPv6 inner frames, one SA's 32-bit number wrapping."""
    pkts, sa_idx, Ls = mixed(np.random.default_rng(size), size, 5)
    run_and_check(gpu_ctx, L.ESP_OUT, SAS5, pkts, sa_idx, Ls, next_seq={0: 0xFFFFFFFE})[1].close()


@pytest.mark.gpu
def test_out_failures(gpu_ctx):
    """Each failure among good packets of the same SA, which get consecutive numbers."""
    rng = np.random.default_rng(3)
    good = lambda: rng.bytes(14) + ipv4(rng, 64)
    v5, long_, ihl4 = bytearray(good()), bytearray(good()), bytearray(good())
    v5[14], long_[16:18], ihl4[14] = 0x55, b"\0\x41", 0x44
    sas = [sa_of(0, mtu=120), None, sa_of(2), sa_of(3, mtu=119)]   # tot is 120
    pkts = [good(), good(), good(), bytes(v5), good(), bytes(long_), bytes(ihl4), good(),
            good(), good(), good()[:30], good()]
    sa_idx = [0, 1, 7, 0, 0, 0, 0, 2, 3, 0, 0, 0]
    res = run_and_check(gpu_ctx, L.ESP_OUT, sas, pkts, sa_idx, [14] * len(pkts))
    res[1].close()
    assert [r[0] for r in res[0]] == [0, 1, 1, 2, 0, 2, 2, 0, 3, 0, 2, 0]
    assert [r[1] for r in res[0]] == [1, 0, 0, 0, 2, 0, 0, 1, 0, 3, 0, 4]


@pytest.mark.gpu
def test_partition_tiles(gpu_ctx):
    """More than two tiles of the radix partition: ranks across tiles. Frame bytes are
    compared for the first and last 16 packets."""
    n = 2 * L.DELIVER_TILE + 5
    rng = np.random.default_rng(9)
    pkts = [rng.bytes(14) + ipv4(rng, 50) for _ in range(n)]
    only = set(range(16)) | set(range(n - 16, n))
    run_and_check(gpu_ctx, L.ESP_OUT, SAS5[:3], pkts, [(i * i) % 3 for i in range(n)], [14] * n,
                  only=only, stride=64)[1].close()


@pytest.mark.gpu
def test_second_call(gpu_ctx):
    """A second call continues the numbers of the first."""
    pkts, sa_idx, Ls = mixed(np.random.default_rng(5), T + 2, 2)
    _, plan, nxt = run_and_check(gpu_ctx, L.ESP_OUT, SAS5[:2], pkts, sa_idx, Ls)
    res = run_and_check(gpu_ctx, L.ESP_OUT, SAS5[:2], pkts[:5], sa_idx[:5], Ls[:5], plan, nxt)[0]
    plan.close()
    assert res[0][1] == 1 + sa_idx.count(sa_idx[0])


def esp_frames(rng, key_len, Lo, ihl=5):
    sa = sa_of(1, key_len)
    opts = rng.bytes(4 * ihl - 20)
    return sa, [encap(rng.bytes(Lo), trailer(ipv4(rng, n), 4), sa, 1000 + n, opts=opts) +
                (rng.bytes(3) if n & 1 else b"") for n in LENGTHS]


@pytest.mark.gpu
@pytest.mark.parametrize("key_len,Lo,ihl", [*itertools.product([16, 24, 32], [14, 18], [5]), (16, 14, 6)])
def test_in_lengths(gpu_ctx, key_len, Lo, ihl):
    """Reference-built ESP frames of every length decrypt to their inner packets."""
    sa, pkts = esp_frames(np.random.default_rng(key_len + Lo + ihl), key_len, Lo, ihl)
    res = run_and_check(gpu_ctx, L.ESP_IN, [None, sa], pkts, [1] * len(pkts), [Lo] * len(pkts))
    res[1].close()
    assert all(r[0] == L.ESP_OK for r in res[0])


def flip(off, bit=1):
    def f(fr, inner):
        fr[off] ^= bit
    return f


def rebuild(pt_edit):
    def f(fr, inner):
        pt = bytearray(trailer(inner, 4))
        pt_edit(pt)
        fr[:] = encap(bytes(fr[:14]), bytes(pt), sa_of(1), 5)
    return f


NEGATIVE = {"ct": (flip(14 + 36 + 40), L.ESP_AUTH), "icv": (flip(-1), L.ESP_AUTH),
            "seq": (flip(14 + 27), L.ESP_AUTH), "spi": (flip(14 + 20), L.ESP_BAD_SPI),
            "mf": (flip(14 + 6, 0x20), L.ESP_BAD_L3), "proto": (flip(14 + 9, 50 ^ 17), L.ESP_BAD_PROTO),
            "short": (lambda fr, inner: fr.__setitem__(slice(16, 18), b"\0\x35"), L.ESP_BAD_LEN),
            "pad": (rebuild(lambda pt: pt.__setitem__(-3, 9)), L.ESP_BAD_PAD),
            "next": (rebuild(lambda pt: pt.__setitem__(-1, 17)), L.ESP_BAD_NEXT)}


@pytest.mark.gpu
@pytest.mark.parametrize("name", NEGATIVE)
def test_in_negative(gpu_ctx, name):
    """One thing wrong in the middle frame of three; its neighbours still decrypt."""
    rng = np.random.default_rng(11)
    inner = ipv4(rng, 60)                     # two pad bytes
    pkts = [bytearray(encap(rng.bytes(14), trailer(inner, 4), sa_of(1), 5)) for _ in range(3)]
    edit, want = NEGATIVE[name]
    edit(pkts[1], inner)
    res = run_and_check(gpu_ctx, L.ESP_IN, [None, sa_of(1)], [bytes(p) for p in pkts], [1] * 3, [14] * 3)
    res[1].close()
    assert [r[0] for r in res[0]] == [0, want, 0]


@pytest.mark.gpu
def test_round_trip(gpu_ctx):
    """in(out(x)) is fr[0, L) | the inner packet, for a mixed batch."""
    pkts, sa_idx, Ls = mixed(np.random.default_rng(21), 2 * T + 5, 5)
    res, plan, _ = run_and_check(gpu_ctx, L.ESP_OUT, SAS5, pkts, sa_idx, Ls)
    plan.close()
    res2, plan, _ = run_and_check(gpu_ctx, L.ESP_IN, SAS5, [r[3] for r in res], sa_idx, Ls)
    plan.close()
    for fr, Lo, r in zip(pkts, Ls, res2):
        n = Lo + (fr[Lo + 2] << 8 | fr[Lo + 3] if fr[Lo] >> 4 == 4 else 40 + (fr[Lo + 4] << 8 | fr[Lo + 5]))
        assert r[0] == L.ESP_OK and r[3] == fr[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("direction", [L.ESP_OUT, L.ESP_IN])
def test_capacity(gpu_ctx, direction):
    """One byte and 1501 bytes short of the full need, and three descriptors short: the
    prefix `copied` says is written, nothing beyond."""
    rng = np.random.default_rng(31)
    pkts, sa_idx, Ls = mixed(rng, T + 3, 5)
    if direction == L.ESP_IN:
        pkts = [r[3] for r in reference(L.ESP_OUT, pkts, SAS5, sa_idx, Ls, [1] * 5)]
    for kw in (dict(capacity=-1), dict(capacity=-1501), dict(max_out=T)):
        run_and_check(gpu_ctx, direction, SAS5, pkts, sa_idx, Ls, **kw)[1].close()


BAD_ARGS = [(dict(num=101), {}), (dict(frames=None), {}), (dict(frames=8), {}), (dict(sa=1), {}),
            (dict(l3_offset=1), {}), (dict(desc=None, stride=0), {}), (dict(desc=None, stride=72), {}),
            ({}, dict(frames=None)), ({}, dict(frames=8)), ({}, dict(desc=None)), ({}, dict(status=None)),
            ({}, dict(seq=None)), ({}, dict(total=None)), ({}, dict(capacity=(1 << 32) + 1)),
            "plan", "src", "dst"]


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAD_ARGS, ids=str)
def test_arguments(gpu_ctx, case):
    """Every -EINVAL of the header returns before a launch: the outputs still hold their
    fill after a sync. An int stands for that offset into the buffer. An empty batch writes
    total only."""
    plan = gpu_ctx.esp(L.ESP_OUT, 4, 100)
    fb, ob = gpu_ctx.buffer(16384), gpu_ctx.buffer(16384)
    ob.upload(np.full(16384, FILL, np.uint8))
    good_s = dict(frames=fb.ptr, desc=fb.ptr, stride=0, num=100, sa=fb.ptr, l3_offset=fb.ptr)
    good_d = dict(frames=ob.ptr, capacity=8192, desc=ob.ptr + 8192, max_out=100, status=ob.ptr + 9216,
                  seq=ob.ptr + 9472, total=ob.ptr + 10240)
    ds, dd = case if isinstance(case, tuple) else ({}, {})
    ds = {k: fb.ptr + v if k in ("frames", "sa", "l3_offset") and v else v for k, v in ds.items()}
    dd = {k: ob.ptr + v if k == "frames" and v else v for k, v in dd.items()}
    s, d = L.odpg_esp_src_t(**{**good_s, **ds}), L.odpg_esp_dst_t(**{**good_d, **dd})
    args = [None if case == "plan" else plan.h, None if case == "src" else C.byref(s),
            None if case == "dst" else C.byref(d)]
    assert L.lib.odpg_esp(*args) == -22
    h = C.c_void_p()
    for direction, nsa, pk in ((2, 4, 100), (0, 0, 100), (0, 2049, 100), (1, 4, (1 << 24) + 1)):
        assert L.lib.odpg_esp_create(gpu_ctx.h, direction, nsa, pk, C.byref(h)) == -22
    assert L.lib.odpg_esp_sa_set(plan.h, 4, C.byref(L.esp_sa(**sa_of(0)))) == -22
    assert L.lib.odpg_esp_sa_set(plan.h, 0, C.byref(L.esp_sa(**sa_of(0, key=bytes(20))))) == -22
    gpu_ctx.sync()
    assert np.all(ob.download(np.uint8, 16384) == FILL)
    s = L.odpg_esp_src_t(**{**good_s, "num": 0})
    assert L.lib.odpg_esp(plan.h, C.byref(s), C.byref(L.odpg_esp_dst_t(**good_d))) == 0
    gpu_ctx.sync()
    after = ob.download(np.uint8, 16384)
    assert after[10240:10264].tobytes() == np.array((0, 0, 0, 0, 0), TOTAL_DT).tobytes()
    after[10240:10264] = FILL
    assert np.all(after == FILL)
    plan.close()
    fb.free()
    ob.free()
