"""Thin Python driver for the odpg.h C-ABI (device buffers, tables, launches).

All compute happens in ``libodpg.so``'s gfx950 kernels; this module moves
numpy arrays in and out of HBM through the library's own helpers.
"""
from __future__ import annotations

import ctypes as C
import sys

import numpy as np

from . import _lib as L

lib = L.lib


class DeviceBuffer:
    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        L.check(lib.odpg_dev_alloc(ctx.h, max(self.nbytes, 16), C.byref(p)), "odpg_dev_alloc")
        self.ptr = p.value

    def upload(self, arr):
        a = np.ascontiguousarray(arr)
        assert a.nbytes <= self.nbytes
        L.check(lib.odpg_memcpy_h2d(self.ctx.h, self.ptr, a.ctypes.data, a.nbytes), "h2d")

    def download(self, dtype, count):
        out = np.empty(count, dtype=dtype)
        if out.nbytes:
            L.check(lib.odpg_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr, out.nbytes),
                    "d2h")
        return out

    def zero(self):
        L.check(lib.odpg_memset_dev(self.ctx.h, self.ptr, 0, self.nbytes), "memset")

    def free(self):
        if self.ptr:
            if self.ctx.h:
                lib.odpg_dev_free(self.ctx.h, self.ptr)
            self.ptr = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.free()
        except Exception:
            pass


def compile_rules(rules):
    """Compiled-table image of `rules` (host only, odpg_rules_compile): the
    bytes a multi-GPU job compiles once and broadcasts."""
    n = C.c_size_t(0)
    rc = lib.odpg_rules_compile(C.byref(rules), None, C.byref(n))
    if rc not in (0, -28):                 # -ENOSPC: size query
        L.check(rc, "odpg_rules_compile")
    buf = (C.c_uint8 * n.value)()
    L.check(lib.odpg_rules_compile(C.byref(rules), buf, C.byref(n)), "odpg_rules_compile")
    return bytes(buf)


class Table:
    def __init__(self, ctx, rules=None, image=None):
        t = C.c_void_p()
        if image is not None:
            b = (C.c_uint8 * len(image)).from_buffer_copy(image)
            L.check(lib.odpg_table_import(ctx.h, b, len(image), C.byref(t)), "odpg_table_import")
        else:
            L.check(lib.odpg_table_create(ctx.h, C.byref(rules), C.byref(t)),
                    "odpg_table_create")
        self.h = t.value
        self.num_cos = lib.odpg_table_num_cos(self.h)
        self.has_cycle = bool(lib.odpg_table_has_cycle(self.h))

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            if self.h:
                lib.odpg_table_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Counters:
    """Sharded device counters of one table layout (odpg.h "sharded
    counters"): launches add into per-workgroup rows; fold() sums them."""

    def __init__(self, ctx, table):
        h = C.c_void_p()
        L.check(lib.odpg_counters_create(ctx.h, table.h, C.byref(h)), "odpg_counters_create")
        self.h = h.value
        self.ctx = ctx
        self.num_cos = table.num_cos
        self.words = 4 + self.num_cos + self.num_cos * L.COS_QUEUE_MAX

    def fold(self):
        """Counts since the last fold: {"pktio": [in_packets, in_octets,
        in_errors, in_discards], "cos": per-CoS packets, "queue": [num_cos,
        COS_QUEUE_MAX] delivered packets}."""
        w = np.zeros(self.words, np.uint64)
        L.check(lib.odpg_counters_fold(self.h, w.ctypes.data_as(C.POINTER(C.c_uint64))),
                "odpg_counters_fold")
        n = self.num_cos
        return {"pktio": w[:4], "cos": w[4:4 + n],
                "queue": w[4 + n:].reshape(n, L.COS_QUEUE_MAX)}

    def close(self):
        if self.h:
            # valid after the context's destroy too: the counters hold a
            # reference to it (odpg.h "object lifetimes")
            lib.odpg_counters_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Deliver:
    """Delivery-list plan of one table layout (include/odpg_deliver.h): from
    verdict words, per destination queue the packet indices in arrival
    order, on the device."""

    def __init__(self, ctx, table, max_pkts):
        h = C.c_void_p()
        L.check(lib.odpg_deliver_create(ctx.h, table.h, max_pkts, C.byref(h)),
                "odpg_deliver_create")
        self.h = h.value
        self.ctx = ctx
        self.max_pkts = max_pkts
        self.num_cos = table.num_cos
        self.num_buckets = lib.odpg_deliver_num_buckets(self.h)

    def queue_base(self, cos):
        """First bucket of CoS `cos` (bucket = queue_base + hash queue)."""
        b = lib.odpg_deliver_queue_base(self.h, cos)
        if b < 0:
            raise L.OdpgError(f"odpg_deliver_queue_base({cos}) failed: {b}")
        return b

    def run_dev(self, out_buf, num, order_buf, offsets_buf):
        """Asynchronous on the context stream: order_buf gets num indices,
        offsets_buf num_buckets + 1 words."""
        L.check(lib.odpg_deliver(self.h, out_buf.ptr, num, order_buf.ptr, offsets_buf.ptr),
                "odpg_deliver")

    def run(self, out_words):
        """Upload verdict words, build the lists, download (order, offsets)."""
        w = np.ascontiguousarray(out_words, dtype=np.uint32)
        ob = self.ctx.buffer(w.nbytes)
        ob.upload(w)
        rb = self.ctx.buffer(w.nbytes)
        fb = self.ctx.buffer(4 * (self.num_buckets + 1))
        self.run_dev(ob, len(w), rb, fb)
        self.ctx.sync()
        res = rb.download(np.uint32, len(w)), fb.download(np.uint32, self.num_buckets + 1)
        for b in (ob, rb, fb):
            b.free()
        return res

    def close(self):
        if self.h:
            # valid after the context's destroy too (odpg.h "object lifetimes")
            lib.odpg_deliver_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Gather:
    """Gather plan (include/odpg_gather.h): the frames of a range of delivery
    buckets written back to back in delivery order, on the device."""

    def __init__(self, ctx, max_pkts):
        h = C.c_void_p()
        L.check(lib.odpg_gather_create(ctx.h, max_pkts, C.byref(h)), "odpg_gather_create")
        self.h = h.value
        self.ctx = ctx
        self.max_pkts = max_pkts

    def run_dev(self, frames_buf, num, order_buf, offsets_buf, b_first, b_last, dst_buf,
                capacity, total_buf, stride=0, desc_buf=None, words_buf=None,
                dst_desc_buf=None, dst_words_buf=None):
        """Asynchronous on the context stream: buckets [b_first, b_last) of
        the lists into dst_buf (capacity bytes), dst_desc_buf / dst_words_buf
        (num entries) and total_buf (odpg_gather_total_t)."""
        s = L.odpg_gather_src_t(frames_buf.ptr, desc_buf.ptr if desc_buf else None, stride, num,
                                words_buf.ptr if words_buf else None)
        d = L.odpg_gather_dst_t(dst_buf.ptr, capacity,
                                dst_desc_buf.ptr if dst_desc_buf else None,
                                dst_words_buf.ptr if dst_words_buf else None, total_buf.ptr)
        L.check(lib.odpg_gather(self.h, C.byref(s), order_buf.ptr, offsets_buf.ptr, b_first,
                                b_last, C.byref(d)), "odpg_gather")

    def run(self, frames, order, offsets, b_first, b_last, stride=0, desc=None, words=None,
            capacity=None, fill=0):
        """Upload, gather, download (frames, desc, words, total). The source
        batch has len(order) frames. Every destination buffer is set to the
        byte `fill` first; frames come back as capacity + 64 bytes (the slack
        frame buffers carry), desc and words with one entry per source frame,
        total as a GATHER_TOTAL_FIELDS record. capacity defaults to the room
        every source frame would need."""
        _, desc_dt = L.np_dtypes()
        num = len(order)
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
            room = int(((desc["len"].astype(np.int64) + 15) // 16 * 16).sum())
        else:
            room = num * stride
        cap = room if capacity is None else int(capacity)
        src = [np.ascontiguousarray(frames, dtype=np.uint8),
               np.ascontiguousarray(order, dtype=np.uint32),
               np.ascontiguousarray(offsets, dtype=np.uint32), desc,
               None if words is None else np.ascontiguousarray(words, dtype=np.uint32)]
        fb, rb, sb, db, wb = (None if a is None else self.ctx.buffer(a.nbytes + 64) for a in src)
        for b, a in zip((fb, rb, sb, db, wb), src):
            if b:
                b.upload(a)
        out = [self.ctx.buffer(cap + 64), self.ctx.buffer(8 * num), self.ctx.buffer(16),
               self.ctx.buffer(4 * num) if wb else None]
        for b in out:
            if b:
                L.check(lib.odpg_memset_dev(self.ctx.h, b.ptr, fill, b.nbytes), "memset")
        self.run_dev(fb, num, rb, sb, b_first, b_last, out[0], cap, out[2], stride, db, wb,
                     out[1], out[3])
        self.ctx.sync()
        res = (out[0].download(np.uint8, cap + 64), out[1].download(desc_dt, num),
               out[3].download(np.uint32, num) if wb else None,
               out[2].download(np.dtype(L.GATHER_TOTAL_FIELDS), 1)[0])
        for b in (fb, rb, sb, db, wb, *out):
            if b:
                b.free()
        return res

    def close(self):
        if self.h:
            # valid after the context's destroy too (odpg.h "object lifetimes")
            lib.odpg_gather_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Lso:
    """Segmentation plan (include/odpg_lso.h): every frame of a batch cut into
    segments of header + payload slice with the profile's header updates, on
    the device. `profiles` is a list of odpg_lso_profile_t (L.lso_profile)."""

    def __init__(self, ctx, profiles, max_pkts):
        h = C.c_void_p()
        arr = (L.odpg_lso_profile_t * max(len(profiles), 1))(*profiles)
        L.check(lib.odpg_lso_create(ctx.h, arr, len(profiles), max_pkts, C.byref(h)),
                "odpg_lso_create")
        self.h = h.value
        self.ctx = ctx
        self.max_pkts = max_pkts

    def run_dev(self, frames_buf, num, dst_buf, capacity, dst_desc_buf, max_segs, seg_first_buf,
                status_buf, total_buf, stride=0, desc_buf=None, opt_buf=None, uniform=None):
        """Asynchronous on the context stream: the segments into dst_buf
        (capacity bytes) and dst_desc_buf (max_segs entries), seg_first_buf
        (num + 1 words), status_buf (num bytes), total_buf (odpg_lso_total_t).
        opt_buf holds num odpg_lso_opt_t; without it `uniform` (an
        odpg_lso_opt_t) applies to every packet."""
        s = L.odpg_lso_src_t(frames_buf.ptr, desc_buf.ptr if desc_buf else None, stride, num,
                             opt_buf.ptr if opt_buf else None, uniform or L.odpg_lso_opt_t())
        d = L.odpg_lso_dst_t(dst_buf.ptr, capacity, dst_desc_buf.ptr, max_segs, 0,
                             seg_first_buf.ptr, status_buf.ptr, total_buf.ptr)
        L.check(lib.odpg_lso(self.h, C.byref(s), C.byref(d)), "odpg_lso")

    def run(self, frames, opts, stride=0, desc=None, capacity=0, max_segs=0, fill=0):
        """Upload, segment, download (frames, desc, seg_first, status, total).
        `opts` is an array of LSO_OPT_FIELDS records, one per packet, or one
        odpg_lso_opt_t for the uniform form. The batch has len(desc) frames,
        or len(frames) // stride. Every destination buffer is set to the byte
        `fill` first; frames come back as capacity + 64 bytes, desc with
        max_segs entries, total as a LSO_TOTAL_FIELDS record."""
        _, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        uniform = opts if isinstance(opts, L.odpg_lso_opt_t) else None
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
        num = len(desc) if desc is not None else len(frames) // stride
        src = [frames, desc,
               None if uniform else np.ascontiguousarray(opts, dtype=np.dtype(L.LSO_OPT_FIELDS))]
        fb, db, ob = (None if a is None else self.ctx.buffer(a.nbytes + 64) for a in src)
        for b, a in zip((fb, db, ob), src):
            if b:
                b.upload(a)
        sizes = (capacity + 64, 8 * max_segs, 4 * (num + 1), num, 24)
        out = [self.ctx.buffer(n) for n in sizes]
        for b in out:
            L.check(lib.odpg_memset_dev(self.ctx.h, b.ptr, fill, b.nbytes), "memset")
        self.run_dev(fb, num, out[0], capacity, out[1], max_segs, out[2], out[3], out[4], stride,
                     db, ob, uniform)
        self.ctx.sync()
        res = (out[0].download(np.uint8, capacity + 64), out[1].download(desc_dt, max_segs),
               out[2].download(np.uint32, num + 1), out[3].download(np.uint8, num),
               out[4].download(np.dtype(L.LSO_TOTAL_FIELDS), 1)[0])
        for b in (fb, db, ob, *out):
            if b:
                b.free()
        return res

    def close(self):
        if self.h:
            # valid after the context's destroy too (odpg.h "object lifetimes")
            lib.odpg_lso_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Reass:
    """Reassembly plan (include/odpg_reass.h): the IPv4 fragments of a batch
    joined into datagrams again on the device, other frames passed through,
    fragments of incomplete datagrams listed as held."""

    def __init__(self, ctx, max_pkts):
        h = C.c_void_p()
        L.check(lib.odpg_reass_create(ctx.h, max_pkts, C.byref(h)), "odpg_reass_create")
        self.h = h.value
        self.ctx = ctx
        self.max_pkts = max_pkts

    def run_dev(self, frames_buf, num, dst_buf, capacity, dst_desc_buf, max_out, origin_buf,
                status_buf, held_buf, held_offsets_buf, total_buf, stride=0, desc_buf=None,
                l3_ptr=None, l3_stride=2, uniform_l3=14):
        """Asynchronous on the context stream: the output frames into dst_buf
        (capacity bytes), dst_desc_buf and origin_buf (max_out entries),
        status_buf (num bytes), held_buf (num words), held_offsets_buf (2
        words), total_buf (odpg_reass_total_t). l3_ptr is the device address
        of the first u16 L3 offset, the next l3_stride bytes on (for a
        classify result: meta_buf.ptr + 14 with sizeof(odpg_meta_t));
        without it uniform_l3 applies to every packet."""
        s = L.odpg_reass_src_t(frames_buf.ptr, desc_buf.ptr if desc_buf else None, stride, num,
                               l3_ptr, l3_stride, uniform_l3, 0)
        d = L.odpg_reass_dst_t(dst_buf.ptr, capacity, dst_desc_buf.ptr, max_out, 0,
                               origin_buf.ptr, status_buf.ptr, held_buf.ptr,
                               held_offsets_buf.ptr, total_buf.ptr)
        L.check(lib.odpg_reass(self.h, C.byref(s), C.byref(d)), "odpg_reass")

    def run(self, frames, l3, stride=0, desc=None, capacity=0, max_out=0, fill=0, l3_stride=2):
        """Upload, reassemble, download (frames, desc, origin, status, held,
        held_offsets, total). `l3` is an int (one L3 offset for all) or an
        array whose bytes hold the u16 offsets l3_stride apart from byte 0.
        The batch has len(desc) frames, or len(frames) // stride. Every
        destination buffer is set to the byte `fill` first; frames come back
        as capacity + 64 bytes, desc and origin with max_out entries, held
        with one word per source frame, total as a REASS_TOTAL_FIELDS record."""
        _, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
        num = len(desc) if desc is not None else len(frames) // stride
        uniform = isinstance(l3, (int, np.integer))
        src = [frames, desc, None if uniform else np.ascontiguousarray(l3)]
        fb, db, lb = (None if a is None else self.ctx.buffer(a.nbytes + 64) for a in src)
        for b, a in zip((fb, db, lb), src):
            if b:
                b.upload(a)
        sizes = (capacity + 64, 8 * max_out, 4 * max_out, num, 4 * num, 8, 24)
        out = [self.ctx.buffer(n) for n in sizes]
        for b in out:
            L.check(lib.odpg_memset_dev(self.ctx.h, b.ptr, fill, b.nbytes), "memset")
        self.run_dev(fb, num, out[0], capacity, out[1], max_out, *out[2:], stride=stride, desc_buf=db,
                     l3_ptr=lb.ptr if lb else None, l3_stride=l3_stride,
                     uniform_l3=int(l3) if uniform else 0)
        self.ctx.sync()
        res = (out[0].download(np.uint8, capacity + 64), out[1].download(desc_dt, max_out),
               out[2].download(np.uint32, max_out), out[3].download(np.uint8, num),
               out[4].download(np.uint32, num), out[5].download(np.uint32, 2),
               out[6].download(np.dtype(L.REASS_TOTAL_FIELDS), 1)[0])
        for b in (fb, db, lb, *out):
            if b:
                b.free()
        return res

    def close(self):
        if self.h:
            # valid after the context's destroy too (odpg.h "object lifetimes")
            lib.odpg_reass_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Switch:
    """L2 learning switch (include/odpg_switch.h): a batch's frames looked up
    in and taught to a MAC table on the device, in index order, with a list
    of frame indices per egress port."""

    def __init__(self, ctx, num_ports, max_pkts):
        h = C.c_void_p()
        L.check(lib.odpg_switch_create(ctx.h, num_ports, max_pkts, C.byref(h)),
                "odpg_switch_create")
        self.h = h.value
        self.ctx = ctx
        self.num_ports = num_ports
        self.max_pkts = max_pkts
        self.table_ptr = lib.odpg_switch_table(self.h)

    def table(self):
        """The MAC table as 65536 u64 entries (bytes 0-5 MAC, 6 port, 7 tick)."""
        t = np.empty(L.SWITCH_TABLE_SIZE, "<u8")
        L.check(lib.odpg_memcpy_d2h(self.ctx.h, t.ctypes.data, self.table_ptr, t.nbytes), "d2h")
        return t

    def set_table(self, entries):
        t = np.ascontiguousarray(entries, dtype="<u8")
        assert len(t) == L.SWITCH_TABLE_SIZE
        L.check(lib.odpg_memcpy_h2d(self.ctx.h, self.table_ptr, t.ctypes.data, t.nbytes), "h2d")

    def run_dev(self, frames_buf, num, cur_tick, out_buf, lists_buf, list_stride,
                port_offsets_buf, total_buf, stride=0, desc_buf=None, port_in_buf=None,
                uniform_port=0):
        """Asynchronous on the context stream: out_buf (num words), lists_buf
        (num_ports x list_stride words), port_offsets_buf (2 x num_ports
        words), total_buf (odpg_switch_total_t). port_in_buf holds a byte per
        packet; without it uniform_port applies to every packet."""
        s = L.odpg_switch_src_t(frames_buf.ptr, desc_buf.ptr if desc_buf else None, stride, num,
                                port_in_buf.ptr if port_in_buf else None, uniform_port)
        d = L.odpg_switch_dst_t(out_buf.ptr, lists_buf.ptr, list_stride, 0,
                                port_offsets_buf.ptr, total_buf.ptr)
        L.check(lib.odpg_switch(self.h, C.byref(s), cur_tick, C.byref(d)), "odpg_switch")

    def run(self, frames, port_in, cur_tick, stride=0, desc=None, list_stride=None, fill=0):
        """Upload, switch, download (out, lists[num_ports, list_stride],
        port_offsets, total). `port_in` is an int (one ingress port for all)
        or a byte per packet. The batch has len(desc) frames, or
        len(frames) // stride. Every destination buffer is set to the byte
        `fill` first; total is a SWITCH_TOTAL_FIELDS record."""
        _, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
        num = len(desc) if desc is not None else len(frames) // stride
        ls = num if list_stride is None else list_stride
        uniform = isinstance(port_in, (int, np.integer))
        src = [frames, desc, None if uniform else np.ascontiguousarray(port_in, dtype=np.uint8)]
        fb, db, pb = (None if a is None else self.ctx.buffer(a.nbytes + 64) for a in src)
        for b, a in zip((fb, db, pb), src):
            if b:
                b.upload(a)
        P = self.num_ports
        out = [self.ctx.buffer(n) for n in (4 * num, 4 * P * ls, 8 * P, 16)]
        for b in out:
            L.check(lib.odpg_memset_dev(self.ctx.h, b.ptr, fill, b.nbytes), "memset")
        self.run_dev(fb, num, cur_tick, out[0], out[1], ls, out[2], out[3], stride=stride,
                     desc_buf=db, port_in_buf=pb, uniform_port=int(port_in) if uniform else 0)
        self.ctx.sync()
        res = (out[0].download(np.uint32, num), out[1].download(np.uint32, P * ls).reshape(P, ls),
               out[2].download(np.uint32, 2 * P),
               out[3].download(np.dtype(L.SWITCH_TOTAL_FIELDS), 1)[0])
        for b in (fb, db, pb, *out):
            if b:
                b.free()
        return res

    def close(self):
        if self.h:
            # valid after the context's destroy too (odpg.h "object lifetimes")
            lib.odpg_switch_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Esp:
    """ESP plan (include/odpg_esp.h): the frames of a batch encapsulated and
    encrypted (ESP_OUT) or authenticated, decrypted and decapsulated (ESP_IN)
    on the device, tunnel mode over IPv4 with AES-GCM."""

    def __init__(self, ctx, direction, max_sas, max_pkts):
        h = C.c_void_p()
        L.check(lib.odpg_esp_create(ctx.h, direction, max_sas, max_pkts, C.byref(h)),
                "odpg_esp_create")
        self.h = h.value
        self.ctx = ctx
        self.dir = direction
        self.max_sas = max_sas
        self.max_pkts = max_pkts
        self.next_seq_ptr = lib.odpg_esp_next_seq(self.h)

    def set_sa(self, index, sa):
        """sa: an odpg_esp_sa_t (L.esp_sa builds one), or None to clear the SA."""
        L.check(lib.odpg_esp_sa_set(self.h, index, C.byref(sa) if sa is not None else None),
                "odpg_esp_sa_set")

    def next_seq(self):
        """The outbound sequence counters, one u64 per SA."""
        t = np.empty(self.max_sas, "<u8")
        L.check(lib.odpg_memcpy_d2h(self.ctx.h, t.ctypes.data, self.next_seq_ptr, t.nbytes), "d2h")
        return t

    def set_next_seq(self, values):
        t = np.ascontiguousarray(values, dtype="<u8")
        assert len(t) == self.max_sas
        L.check(lib.odpg_memcpy_h2d(self.ctx.h, self.next_seq_ptr, t.ctypes.data, t.nbytes), "h2d")

    def run_dev(self, frames_buf, num, dst_buf, capacity, dst_desc_buf, max_out, status_buf,
                seq_buf, total_buf, stride=0, desc_buf=None, sa_buf=None, uniform_sa=0,
                l3_buf=None, uniform_l3=14):
        """Asynchronous on the context stream: the output frames into dst_buf
        (capacity bytes), dst_desc_buf (max_out entries), status_buf (num
        bytes), seq_buf (num words), total_buf (odpg_esp_total_t). sa_buf and
        l3_buf hold a u16 per packet; without them uniform_sa / uniform_l3
        apply to every packet."""
        s = L.odpg_esp_src_t(frames_buf.ptr, desc_buf.ptr if desc_buf else None, stride, num,
                             sa_buf.ptr if sa_buf else None, l3_buf.ptr if l3_buf else None,
                             uniform_sa, uniform_l3, 0)
        d = L.odpg_esp_dst_t(dst_buf.ptr, capacity, dst_desc_buf.ptr, max_out, 0, status_buf.ptr,
                             seq_buf.ptr, total_buf.ptr)
        L.check(lib.odpg_esp(self.h, C.byref(s), C.byref(d)), "odpg_esp")

    def run(self, frames, sa, l3, stride=0, desc=None, capacity=0, max_out=0, fill=0):
        """Upload, run, download (frames, desc, status, seq, total). `sa` and
        `l3` are an int (one for all) or a u16 per packet. The batch has
        len(desc) frames, or len(frames) // stride. Every destination buffer
        is set to the byte `fill` first; frames come back as capacity + 64
        bytes, desc with max_out entries, total as an ESP_TOTAL_FIELDS record."""
        _, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
        num = len(desc) if desc is not None else len(frames) // stride
        usa, ul3 = (isinstance(v, (int, np.integer)) for v in (sa, l3))
        src = [frames, desc, None if usa else np.ascontiguousarray(sa, dtype="<u2"),
               None if ul3 else np.ascontiguousarray(l3, dtype="<u2")]
        fb, db, sb, lb = (None if a is None else self.ctx.buffer(a.nbytes + 64) for a in src)
        for b, a in zip((fb, db, sb, lb), src):
            if b:
                b.upload(a)
        out = [self.ctx.buffer(n) for n in (capacity + 64, 8 * max_out, num, 4 * num, 24)]
        for b in out:
            L.check(lib.odpg_memset_dev(self.ctx.h, b.ptr, fill, b.nbytes), "memset")
        self.run_dev(fb, num, out[0], capacity, out[1], max_out, out[2], out[3], out[4],
                     stride=stride, desc_buf=db, sa_buf=sb, uniform_sa=int(sa) if usa else 0,
                     l3_buf=lb, uniform_l3=int(l3) if ul3 else 0)
        self.ctx.sync()
        res = (out[0].download(np.uint8, capacity + 64), out[1].download(desc_dt, max_out),
               out[2].download(np.uint8, num), out[3].download(np.uint32, num),
               out[4].download(np.dtype(L.ESP_TOTAL_FIELDS), 1)[0])
        for b in (fb, db, sb, lb, *out):
            if b:
                b.free()
        return res

    def close(self):
        if self.h:
            # valid after the context's destroy too (odpg.h "object lifetimes")
            lib.odpg_esp_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass


class Context:
    def __init__(self, device=0, stream=None):
        n = lib.odpg_device_count()
        if n <= 0:
            raise RuntimeError("no HIP device visible (odpg_device_count() == 0)")
        h = C.c_void_p()
        L.check(lib.odpg_ctx_create(device, stream, C.byref(h)), "odpg_ctx_create")
        self.h = h.value
        self.device = device

    def close(self):
        if self.h:
            lib.odpg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass

    def set_kernel_mode(self, mode):
        """0 auto, 1 wave-cooperative walk, 2 evaluate-all, 3 hash walk (same results)."""
        L.check(lib.odpg_ctx_set_kernel_mode(self.h, mode), "odpg_ctx_set_kernel_mode")

    def sync(self):
        L.check(lib.odpg_ctx_sync(self.h), "odpg_ctx_sync")

    def buffer(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def table(self, rules=None, image=None):
        return Table(self, rules, image)

    def counters(self, table):
        return Counters(self, table)

    def deliver(self, table, max_pkts=1 << 20):
        return Deliver(self, table, max_pkts)

    def gather(self, max_pkts=1 << 20):
        return Gather(self, max_pkts)

    def lso(self, profiles, max_pkts=1 << 16):
        return Lso(self, profiles, max_pkts)

    def reass(self, max_pkts=1 << 16):
        return Reass(self, max_pkts)

    def switch(self, num_ports, max_pkts=1 << 20):
        return Switch(self, num_ports, max_pkts)

    def esp(self, direction, max_sas, max_pkts=1 << 20):
        return Esp(self, direction, max_sas, max_pkts)

    def classify_dev(self, table, frames_buf, num, stride=0, desc_buf=None, opt=0,
                     layer=L.LAYER_ALL, classify=True, out_buf=None, mark_buf=None,
                     meta_buf=None, stats_buf=None, counters=None):
        b = L.odpg_batch_t(frames_buf.ptr, desc_buf.ptr if desc_buf else None, stride, num,
                           opt, layer, int(bool(classify)))
        r = L.odpg_result_t(out_buf.ptr if out_buf else None,
                            mark_buf.ptr if mark_buf else None,
                            meta_buf.ptr if meta_buf else None,
                            stats_buf.ptr if stats_buf else None,
                            counters.h if counters else None)
        L.check(lib.odpg_classify(self.h, table.h, C.byref(b), C.byref(r)), "odpg_classify")

    def classify(self, table, frames, num, stride=0, desc=None, opt=0, layer=L.LAYER_ALL,
                 classify=True, want_mark=True, want_meta=True, want_stats=True,
                 counters=None):
        """Upload host arrays, classify on the GPU, download results. With
        `counters` the launch adds into those (want_stats is ignored)."""
        if counters is not None:
            want_stats = False
        meta_dt, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        fb = self.buffer(frames.nbytes + 64)
        fb.upload(frames)
        db = None
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
            db = self.buffer(desc.nbytes)
            db.upload(desc)
        ob = self.buffer(4 * num)
        mb = self.buffer(2 * num) if want_mark else None
        eb = self.buffer(24 * num) if want_meta else None
        nst = 4 + table.num_cos
        sb = self.buffer(8 * nst) if want_stats else None
        if sb:
            sb.zero()
        self.classify_dev(table, fb, num, stride, db, opt, layer, classify, ob, mb, eb, sb,
                          counters)
        self.sync()
        res = {"out": ob.download(np.uint32, num)}
        if mb:
            res["mark"] = mb.download(np.uint16, num)
        if eb:
            res["meta"] = eb.download(meta_dt, num)
        if sb:
            res["stats"] = sb.download(np.uint64, nst)
        for b in (fb, db, ob, mb, eb, sb):
            if b:
                b.free()
        return res

    def tx_prepare(self, frames, num, stride=0, desc=None, meta=None, pktout_cfg=0,
                   pktout_capa=L.PKTOUT_LOOP_CAPA, hash_proto=0, num_qs=1, index=0):
        """loopback_send()'s checksum insertion + loop queue pick on the GPU
        (include/odpg_tx.h). Returns (out words, rewritten frames)."""
        _, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        fb = self.buffer(frames.nbytes + 64)
        fb.upload(frames)
        db = mb = None
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
            db = self.buffer(desc.nbytes)
            db.upload(desc)
        if meta is not None:
            meta = np.ascontiguousarray(meta, dtype=np.dtype(L.TX_META_FIELDS))
            mb = self.buffer(meta.nbytes)
            mb.upload(meta)
        ob = self.buffer(4 * num)
        b = L.odpg_tx_batch_t(fb.ptr, db.ptr if db else None, stride, num,
                              mb.ptr if mb else None)
        c = L.odpg_tx_cfg_t(pktout_cfg, pktout_capa, hash_proto, num_qs, index, 0)
        L.check(lib.odpg_tx_prepare(self.h, C.byref(b), C.byref(c), ob.ptr), "odpg_tx_prepare")
        self.sync()
        out = ob.download(np.uint32, num)
        fr = fb.download(np.uint8, frames.nbytes)
        for x in (fb, db, mb, ob):
            if x:
                x.free()
        return out, fr

    def classify_host(self, table, frames, num, stride=0, desc=None, opt=0,
                      layer=L.LAYER_ALL, classify=True, chunk=0, want_mark=False,
                      want_meta=False, want_stats=True):
        meta_dt, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        dptr = None
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
            dptr = desc.ctypes.data
        out = np.zeros(num, np.uint32)
        mark = np.zeros(num, np.uint16) if want_mark else None
        meta = np.zeros(num, meta_dt) if want_meta else None
        stats = np.zeros(4 + table.num_cos, np.uint64) if want_stats else None
        b = L.odpg_batch_t(frames.ctypes.data, dptr, stride, num, opt, layer,
                           int(bool(classify)))
        r = L.odpg_result_t(out.ctypes.data, mark.ctypes.data if mark is not None else None,
                            meta.ctypes.data if meta is not None else None,
                            stats.ctypes.data if stats is not None else None)
        L.check(lib.odpg_classify_host(self.h, table.h, C.byref(b), C.byref(r), chunk),
                "odpg_classify_host")
        res = {"out": out}
        if mark is not None:
            res["mark"] = mark
        if meta is not None:
            res["meta"] = meta
        if stats is not None:
            res["stats"] = stats
        return res


def group_range(num, n, member):
    """odpg_group_range: member's packet range [lo, hi) of a num-packet batch
    over n members (host arithmetic, no device)."""
    lo, hi = C.c_uint32(), C.c_uint32()
    lib.odpg_group_range(num, n, member, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


class Group:
    """Several device contexts classifying one batch by packet range
    (include/odpg_group.h): the table compiled once and imported per member,
    per-member counters summed when folded."""

    def __init__(self, devices):
        devs = (C.c_int * len(devices))(*devices)
        h = C.c_void_p()
        L.check(lib.odpg_group_create(devs, len(devices), C.byref(h)), "odpg_group_create")
        self.h = h.value
        self.n = len(devices)
        self.num_cos = 0

    def close(self):
        if self.h:
            lib.odpg_group_destroy(self.h)
            self.h = None

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            self.close()
        except Exception:
            pass

    def load(self, rules):
        L.check(lib.odpg_group_load(self.h, C.byref(rules)), "odpg_group_load")
        self.num_cos = lib.odpg_table_num_cos(lib.odpg_group_table(self.h, 0))

    def ctx_handle(self, member):
        return lib.odpg_group_ctx(self.h, member)

    def classify_host(self, frames, num, stride=0, desc=None, opt=0, layer=L.LAYER_ALL,
                      counted=False, chunk=0):
        """Host arrays in, verdict words out (odpg_group_classify_host)."""
        _, desc_dt = L.np_dtypes()
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        dptr = None
        if desc is not None:
            desc = np.ascontiguousarray(desc, dtype=desc_dt)
            dptr = desc.ctypes.data
        out = np.zeros(num, np.uint32)
        b = L.odpg_batch_t(frames.ctypes.data, dptr, stride, num, opt, layer, 1)
        r = L.odpg_result_t(out.ctypes.data, None, None, None, None)
        L.check(lib.odpg_group_classify_host(self.h, C.byref(b), C.byref(r), int(counted), chunk),
                "odpg_group_classify_host")
        return out

    def classify_shards(self, frames, num, stride, opt=0, counted=False, desc=None):
        """Device-resident shards: member i's range uploaded to its own HBM
        (fixed stride: its frames; with descriptors: the whole frame buffer
        and its range's descriptors, offsets relative to that buffer), all
        members launched (odpg_group_classify), synced, verdicts gathered."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        B = (L.odpg_batch_t * self.n)()
        R = (L.odpg_result_t * self.n)()
        bufs = []
        for i in range(self.n):
            lo, hi = group_range(num, self.n, i)
            ctx = _CtxView(self.ctx_handle(i))
            db = None
            if desc is None:
                fb = DeviceBuffer(ctx, max(16, (hi - lo) * stride))
                if hi > lo:
                    fb.upload(frames[lo * stride:hi * stride])
            else:
                fb = DeviceBuffer(ctx, max(16, frames.nbytes))
                fb.upload(frames)
                d = np.ascontiguousarray(desc[lo:hi])
                db = DeviceBuffer(ctx, max(16, d.nbytes))
                if hi > lo:
                    db.upload(d)
            ob = DeviceBuffer(ctx, max(16, 4 * (hi - lo)))
            B[i] = L.odpg_batch_t(fb.ptr, db.ptr if db else None, 0 if db else stride, hi - lo,
                                  opt, L.LAYER_ALL, 1)
            R[i] = L.odpg_result_t(ob.ptr, None, None, None, None)
            bufs.append((lo, hi, fb, ob, db))
        L.check(lib.odpg_group_classify(self.h, B, R, int(counted)), "odpg_group_classify")
        L.check(lib.odpg_group_sync(self.h), "odpg_group_sync")
        out = np.zeros(num, np.uint32)
        for lo, hi, fb, ob, db in bufs:
            if hi > lo:
                out[lo:hi] = ob.download(np.uint32, hi - lo)
            fb.free()
            ob.free()
            if db:
                db.free()
        return out

    def fold(self):
        w = np.zeros(4 + self.num_cos + self.num_cos * L.COS_QUEUE_MAX, np.uint64)
        L.check(lib.odpg_group_counters_fold(self.h, w.ctypes.data_as(C.POINTER(C.c_uint64))),
                "odpg_group_counters_fold")
        n = self.num_cos
        return {"pktio": w[:4], "cos": w[4:4 + n],
                "queue": w[4 + n:].reshape(n, L.COS_QUEUE_MAX)}


class _CtxView:
    """A member context of a Group, for DeviceBuffer (not owned)."""

    def __init__(self, h):
        self.h = h


class Forwarder:
    """example/l3fwd forwarding table on the device (include/odpg_fwd.h)."""

    def __init__(self, ctx, routes, mode=L.FWD_HASH, port_mac=None, dest_mac=None, num_ports=4):
        self.ctx = ctx
        self.routes = make_routes(routes)
        self.param = make_fwd_param(mode, num_ports, port_mac, dest_mac)
        h = C.c_void_p()
        L.check(lib.odpg_fwd_create(ctx.h, self.routes, len(self.routes), C.byref(self.param),
                                    C.byref(h)), "odpg_fwd_create")
        self.h = h.value

    def __del__(self):
        if sys.is_finalizing():   # the HIP runtime may be torn down already
            return
        try:
            if self.h:
                lib.odpg_fwd_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def run_dev(self, frames_buf, stride, num, out_buf, src_port=0, error_check=False):
        b = L.odpg_fwd_batch_t(frames_buf.ptr, stride, num, src_port, int(bool(error_check)))
        L.check(lib.odpg_l3fwd(self.ctx.h, self.h, C.byref(b), out_buf.ptr), "odpg_l3fwd")

    def run(self, frames, stride, num, src_port=0, error_check=False):
        """Upload, forward, download: returns (out_port int32[num], frames)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        fb = self.ctx.buffer(frames.nbytes + 64)
        fb.upload(frames)
        ob = self.ctx.buffer(4 * num)
        self.run_dev(fb, stride, num, ob, src_port, error_check)
        self.ctx.sync()
        out = ob.download(np.int32, num)
        fr = fb.download(np.uint8, frames.nbytes)
        fb.free()
        ob.free()
        return out, fr


def make_routes(routes):
    """[(addr, depth, oif_id, src_mac, dst_mac), ...] -> ctypes odpg_route_t array."""
    arr = (L.odpg_route_t * len(routes))()
    for k, (addr, depth, oif, smac, dmac) in enumerate(routes):
        arr[k].addr, arr[k].depth, arr[k].oif_id = addr, depth, oif
        for j in range(6):
            arr[k].src_mac[j] = smac[j]
            arr[k].dst_mac[j] = dmac[j]
    return arr


def make_fwd_param(mode, num_ports, port_mac=None, dest_mac=None):
    p = L.odpg_fwd_param_t()
    p.mode, p.num_ports = mode, num_ports
    for i in range(L.FWD_MAX_PORTS):
        pm = port_mac[i] if port_mac and i < len(port_mac) else [0x02, 0, 0, 0xAA, 0, i]
        dm = dest_mac[i] if dest_mac and i < len(dest_mac) else [0x02, 0, 0, 0xBB, 0, i]
        for j in range(6):
            p.port_mac[i][j] = pm[j]
            p.dest_mac[i][j] = dm[j]
    return p
