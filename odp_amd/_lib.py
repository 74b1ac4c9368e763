"""ctypes binding of the product library ``odp_amd/lib/libodpg.so``.

Declares every entry point of ``include/odpg.h`` and ``include/odp_cls.h``
with its C signature. Loading fails loudly if the library has not been built:
there is no Python / CPU fallback for the classifier.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# ODPG_LIB selects another build of the same library (A/B kernel experiments)
LIB_PATH = os.environ.get("ODPG_LIB") or os.path.join(_HERE, "lib", "libodpg.so")

# ---- constants mirrored from include/odpg.h -------------------------------
ABI_VERSION = 2
COS_QUEUE_MAX = 32
ODPG_COS_NONE = 0xFFFF
ODPG_COS_PDROP = 0xFFFE
ODPG_COS_LOOP = 0xFFFD
ODPG_COS_NOCLS = 0xFFFC
ODPG_OUT_ERROR = 1 << 20
ODPG_OUT_CLS_DROP = 1 << 21
ODPG_OUT_MARK_VALID = 1 << 22
ODPG_OUT_PARSE_ERR = 1 << 23
ODPG_CHKSUM_UNKNOWN, ODPG_CHKSUM_OK, ODPG_CHKSUM_BAD = 0, 1, 2

PKTIN_TS_ALL = 1 << 0
PKTIN_TS_PTP = 1 << 1
PKTIN_IPV4_CHKSUM = 1 << 2
PKTIN_UDP_CHKSUM = 1 << 3
PKTIN_TCP_CHKSUM = 1 << 4
PKTIN_SCTP_CHKSUM = 1 << 5
PKTIN_DROP_IPV4_ERR = 1 << 6
PKTIN_DROP_IPV6_ERR = 1 << 7
PKTIN_DROP_UDP_ERR = 1 << 8
PKTIN_DROP_TCP_ERR = 1 << 9
PKTIN_DROP_SCTP_ERR = 1 << 10

LAYER_NONE, LAYER_L2, LAYER_L3, LAYER_L4, LAYER_ALL = range(5)


def out_cos(w):
    return w & 0xFFFF


def out_l3(w):
    return (w >> 16) & 3


def out_l4(w):
    return (w >> 18) & 3


def out_hashq(w):
    return (w >> 24) & 31


# ---- structs ---------------------------------------------------------------
class odpg_term_t(C.Structure):
    _fields_ = [("term", C.c_uint32), ("val_sz", C.c_uint32), ("offset", C.c_uint32),
                ("value", C.c_uint8 * 16), ("mask", C.c_uint8 * 16)]


class odpg_pmr_t(C.Structure):
    _fields_ = [("num_terms", C.c_uint32), ("mark", C.c_uint32), ("terms", odpg_term_t * 8)]


class odpg_cos_t(C.Structure):
    _fields_ = [("valid", C.c_uint32), ("action", C.c_uint32), ("num_queue", C.c_uint32),
                ("hash_proto", C.c_uint32), ("stats_enable", C.c_uint32),
                ("num_rule", C.c_uint32), ("rule_start", C.c_uint32)]


class odpg_rules_t(C.Structure):
    _fields_ = [("num_cos", C.c_uint32), ("cos", C.POINTER(odpg_cos_t)),
                ("num_pmr", C.c_uint32), ("pmr", C.POINTER(odpg_pmr_t)),
                ("num_slots", C.c_uint32), ("rule_pmr", C.POINTER(C.c_uint32)),
                ("rule_dst", C.POINTER(C.c_uint32)),
                ("default_cos", C.c_int32), ("error_cos", C.c_int32)]


class odpg_desc_t(C.Structure):
    _fields_ = [("offset", C.c_uint32), ("len", C.c_uint32)]


class odpg_meta_t(C.Structure):
    _fields_ = [("input_flags", C.c_uint64), ("flags", C.c_uint32),
                ("l2_offset", C.c_uint16), ("l3_offset", C.c_uint16),
                ("l4_offset", C.c_uint16), ("cls_mark", C.c_uint16),
                ("reserved", C.c_uint32)]


class odpg_batch_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("pktin_opt", C.c_uint64), ("layer", C.c_uint32),
                ("classify", C.c_uint32)]


class odpg_result_t(C.Structure):
    _fields_ = [("out", C.c_void_p), ("mark", C.c_void_p), ("meta", C.c_void_p),
                ("stats", C.c_void_p), ("counters", C.c_void_p)]


# ---- include/odpg_fwd.h -----------------------------------------------------
FWD_HASH, FWD_LPM = 0, 1
FWD_MAX_ROUTES = 32
FWD_MAX_PORTS = 32


class odpg_route_t(C.Structure):
    _fields_ = [("addr", C.c_uint32), ("depth", C.c_uint32), ("oif_id", C.c_int32),
                ("src_mac", C.c_uint8 * 6), ("dst_mac", C.c_uint8 * 6)]


class odpg_fwd_param_t(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("num_ports", C.c_uint32),
                ("port_mac", (C.c_uint8 * 6) * FWD_MAX_PORTS),
                ("dest_mac", (C.c_uint8 * 6) * FWD_MAX_PORTS)]


class odpg_fwd_batch_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("stride", C.c_uint32), ("num", C.c_uint32),
                ("src_port", C.c_int32), ("error_check", C.c_uint32)]


# ---- include/odpg_tx.h ------------------------------------------------------
PKTOUT_IPV4_CHKSUM, PKTOUT_UDP_CHKSUM = 1 << 5, 1 << 6
PKTOUT_TCP_CHKSUM, PKTOUT_SCTP_CHKSUM = 1 << 7, 1 << 8
PKTOUT_LOOP_CAPA = PKTOUT_IPV4_CHKSUM | PKTOUT_UDP_CHKSUM | PKTOUT_TCP_CHKSUM | PKTOUT_SCTP_CHKSUM
HASH_IPV4_UDP, HASH_IPV4_TCP, HASH_IPV4 = 1, 2, 4
HASH_IPV6_UDP, HASH_IPV6_TCP, HASH_IPV6 = 8, 16, 32
TX_L3_CHKSUM_SET, TX_L3_CHKSUM, TX_L4_CHKSUM_SET, TX_L4_CHKSUM = 1, 2, 4, 8
TX_HAS_IPV4, TX_HAS_IPV6, TX_HAS_UDP, TX_HAS_TCP = 1 << 8, 1 << 9, 1 << 10, 1 << 11
TX_OUT_IPV4, TX_OUT_UDP, TX_OUT_TCP, TX_OUT_SCTP = 1 << 16, 1 << 17, 1 << 18, 1 << 19
OFFSET_INVALID = 0xFFFF


class odpg_tx_batch_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("meta", C.c_void_p)]


class odpg_tx_cfg_t(C.Structure):
    _fields_ = [("pktout_cfg", C.c_uint64), ("pktout_capa", C.c_uint64),
                ("hash_proto", C.c_uint32), ("num_qs", C.c_uint32), ("index", C.c_uint32),
                ("reserved", C.c_uint32)]


TX_META_FIELDS = [("l3_offset", "<u2"), ("l4_offset", "<u2"), ("flags", "<u4")]   # 8 B


# ---- include/odpg_deliver.h -------------------------------------------------
DELIVER_TILE = 4096      # ODPG_DELIVER_TILE: packets one workgroup ranks


def deliver_pktin(nbuckets):
    return nbuckets - 2


def deliver_free(nbuckets):
    return nbuckets - 1


# ---- include/odpg_gather.h --------------------------------------------------
GATHER_TILE = 1024       # ODPG_GATHER_TILE: positions one workgroup handles


class odpg_gather_src_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("words", C.c_void_p)]


class odpg_gather_total_t(C.Structure):
    _fields_ = [("num", C.c_uint32), ("copied", C.c_uint32), ("bytes", C.c_uint64)]


class odpg_gather_dst_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("capacity", C.c_uint64), ("desc", C.c_void_p),
                ("words", C.c_void_p), ("total", C.c_void_p)]


GATHER_TOTAL_FIELDS = [("num", "<u4"), ("copied", "<u4"), ("bytes", "<u8")]   # 16 B


# ---- include/odpg_lso.h -----------------------------------------------------
LSO_TILE = 64            # ODPG_LSO_TILE: packets one copy workgroup handles
LSO_PROTO_CUSTOM, LSO_PROTO_IPV4 = 1, 2
LSO_ADD_SEGMENT_NUM, LSO_WRITE_BITS = 1, 5
LSO_MAX_CUSTOM, LSO_MAX_PROFILES, LSO_MAX_SEGMENTS, LSO_MAX_PAYLOAD_OFFSET = 8, 16, 64, 128
(LSO_OK, LSO_BAD_PROFILE, LSO_BAD_OFFSET, LSO_BAD_L3, LSO_BAD_PAYLOAD, LSO_TOO_MANY,
 LSO_BAD_IHL, LSO_BAD_FIELD) = range(8)


class odpg_lso_bits_t(C.Structure):
    _fields_ = [("mask", C.c_uint8), ("value", C.c_uint8)]


class odpg_lso_field_t(C.Structure):
    _fields_ = [("mod_op", C.c_uint8), ("size", C.c_uint8), ("offset", C.c_uint16),
                ("first", odpg_lso_bits_t), ("middle", odpg_lso_bits_t),
                ("last", odpg_lso_bits_t), ("reserved", C.c_uint16)]


class odpg_lso_profile_t(C.Structure):
    _fields_ = [("proto", C.c_uint32), ("num_custom", C.c_uint32),
                ("field", odpg_lso_field_t * LSO_MAX_CUSTOM)]


class odpg_lso_opt_t(C.Structure):
    _fields_ = [("payload_offset", C.c_uint16), ("max_payload_len", C.c_uint16),
                ("l3_offset", C.c_uint16), ("profile", C.c_uint8), ("reserved", C.c_uint8)]


class odpg_lso_src_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("opt", C.c_void_p), ("uniform", odpg_lso_opt_t)]


class odpg_lso_total_t(C.Structure):
    _fields_ = [("num_segs", C.c_uint32), ("copied", C.c_uint32), ("first_bad", C.c_uint32),
                ("reserved", C.c_uint32), ("bytes", C.c_uint64)]


class odpg_lso_dst_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("capacity", C.c_uint64), ("desc", C.c_void_p),
                ("max_segs", C.c_uint32), ("reserved", C.c_uint32), ("seg_first", C.c_void_p),
                ("status", C.c_void_p), ("total", C.c_void_p)]


LSO_OPT_FIELDS = [("payload_offset", "<u2"), ("max_payload_len", "<u2"), ("l3_offset", "<u2"),
                  ("profile", "u1"), ("reserved", "u1")]                       # 8 B
LSO_TOTAL_FIELDS = [("num_segs", "<u4"), ("copied", "<u4"), ("first_bad", "<u4"),
                    ("reserved", "<u4"), ("bytes", "<u8")]                     # 24 B


def lso_profile(proto, fields=()):
    """odpg_lso_profile_t from (mod_op, offset, size[, first, middle, last]) tuples;
    first / middle / last are (mask, value) pairs of WRITE_BITS."""
    p = odpg_lso_profile_t(proto=proto, num_custom=len(fields))
    for f, (op, off, size, *bits) in zip(p.field, fields):
        f.mod_op, f.offset, f.size = op, off, size
        for name, (m, v) in zip(("first", "middle", "last"), bits):
            setattr(f, name, odpg_lso_bits_t(m, v))
    return p


# ---- include/odpg_reass.h ---------------------------------------------------
REASS_TILE = 64          # ODPG_REASS_TILE: packets one copy workgroup handles
REASS_WHOLE, REASS_JOINED, REASS_HELD, REASS_BAD = range(4)


class odpg_reass_src_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("l3_offset", C.c_void_p), ("l3_stride", C.c_uint32),
                ("uniform_l3", C.c_uint16), ("reserved", C.c_uint16)]


class odpg_reass_total_t(C.Structure):
    _fields_ = [("num_out", C.c_uint32), ("copied", C.c_uint32), ("num_held", C.c_uint32),
                ("num_bad", C.c_uint32), ("bytes", C.c_uint64)]


class odpg_reass_dst_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("capacity", C.c_uint64), ("desc", C.c_void_p),
                ("max_out", C.c_uint32), ("reserved", C.c_uint32), ("origin", C.c_void_p),
                ("status", C.c_void_p), ("held", C.c_void_p), ("held_offsets", C.c_void_p),
                ("total", C.c_void_p)]


REASS_TOTAL_FIELDS = [("num_out", "<u4"), ("copied", "<u4"), ("num_held", "<u4"),
                      ("num_bad", "<u4"), ("bytes", "<u8")]                    # 24 B


# ---- include/odpg_switch.h --------------------------------------------------
SWITCH_TILE = 256        # ODPG_SWITCH_TILE: packets one resolve / list workgroup handles
SWITCH_UNICAST, SWITCH_FLOOD, SWITCH_DROP_FRAME, SWITCH_DROP_PORT = range(4)
SWITCH_MAX_PORTS = 32
SWITCH_TABLE_SIZE = 65536
SWITCH_AGING_TIME = 5


class odpg_switch_src_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("port_in", C.c_void_p), ("uniform_port", C.c_uint8),
                ("reserved", C.c_uint8 * 7)]


class odpg_switch_dst_t(C.Structure):
    _fields_ = [("out", C.c_void_p), ("lists", C.c_void_p), ("list_stride", C.c_uint32),
                ("reserved", C.c_uint32), ("port_offsets", C.c_void_p), ("total", C.c_void_p)]


SWITCH_TOTAL_FIELDS = [("unicast", "<u4"), ("flooded", "<u4"), ("dropped", "<u4"),
                       ("entries", "<u4")]                                     # 16 B


# ---- include/odpg_esp.h -----------------------------------------------------
ESP_TILE = 16            # ODPG_ESP_TILE: packets one crypt workgroup handles
ESP_MAX_SAS = 2048
ESP_OUT, ESP_IN = 0, 1
(ESP_OK, ESP_NO_SA, ESP_BAD_L3, ESP_MTU, ESP_BAD_PROTO, ESP_BAD_SPI, ESP_BAD_LEN, ESP_AUTH,
 ESP_BAD_PAD, ESP_BAD_NEXT) = range(10)


class odpg_esp_sa_t(C.Structure):
    _fields_ = [("spi", C.c_uint32), ("key", C.c_uint8 * 32), ("key_len", C.c_uint32),
                ("salt", C.c_uint8 * 4), ("tun_src", C.c_uint8 * 4), ("tun_dst", C.c_uint8 * 4),
                ("ttl", C.c_uint8), ("dscp", C.c_uint8), ("df", C.c_uint8),
                ("copy_dscp", C.c_uint8), ("copy_df", C.c_uint8), ("reserved", C.c_uint8),
                ("mtu", C.c_uint16)]


class odpg_esp_src_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("stride", C.c_uint32),
                ("num", C.c_uint32), ("sa", C.c_void_p), ("l3_offset", C.c_void_p),
                ("uniform_sa", C.c_uint16), ("uniform_l3", C.c_uint16), ("reserved", C.c_uint32)]


class odpg_esp_dst_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("capacity", C.c_uint64), ("desc", C.c_void_p),
                ("max_out", C.c_uint32), ("reserved", C.c_uint32), ("status", C.c_void_p),
                ("seq", C.c_void_p), ("total", C.c_void_p)]


ESP_TOTAL_FIELDS = [("num_out", "<u4"), ("copied", "<u4"), ("first_bad", "<u4"),
                    ("reserved", "<u4"), ("bytes", "<u8")]                     # 24 B


def esp_sa(spi, key, salt, tun_src=bytes(4), tun_dst=bytes(4), ttl=64, dscp=0, df=0,
           copy_dscp=0, copy_df=0, mtu=0xFFFF):
    """odpg_esp_sa_t from bytes objects and integers."""
    sa = odpg_esp_sa_t(spi=spi, key_len=len(key), ttl=ttl, dscp=dscp, df=df,
                       copy_dscp=copy_dscp, copy_df=copy_df, mtu=mtu)
    C.memmove(sa.key, bytes(key), min(len(key), 32))
    for name, v in (("salt", salt), ("tun_src", tun_src), ("tun_dst", tun_dst)):
        C.memmove(getattr(sa, name), bytes(v), 4)
    return sa


# ---- include/odpg_pcap.h ----------------------------------------------------
class odpg_capture_t(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("desc", C.c_void_p), ("num", C.c_uint32),
                ("bytes", C.c_uint64)]


# numpy dtypes with the same layout
def np_dtypes():
    import numpy as np
    meta = np.dtype([("input_flags", "<u8"), ("flags", "<u4"), ("l2_offset", "<u2"),
                     ("l3_offset", "<u2"), ("l4_offset", "<u2"), ("cls_mark", "<u2"),
                     ("reserved", "<u4")])
    desc = np.dtype([("offset", "<u4"), ("len", "<u4")])
    assert meta.itemsize == C.sizeof(odpg_meta_t) == 24
    assert desc.itemsize == C.sizeof(odpg_desc_t) == 8
    return meta, desc


# odp_cls.h structs
class odp_pmr_param_t(C.Structure):
    _fields_ = [("term", C.c_int), ("range_term", C.c_int),
                ("value", C.c_void_p), ("mask", C.c_void_p),
                ("val_sz", C.c_uint32), ("offset", C.c_uint32)]


class odp_pmr_create_opt_t(C.Structure):
    _fields_ = [("terms", C.POINTER(odp_pmr_param_t)), ("num_terms", C.c_int),
                ("mark", C.c_uint64)]


class odp_schedule_param_t(C.Structure):
    _fields_ = [("prio", C.c_int), ("sync", C.c_int), ("group", C.c_int),
                ("lock_count", C.c_uint32)]


class odp_queue_param_t(C.Structure):
    _fields_ = [("type", C.c_int), ("enq_mode", C.c_int), ("deq_mode", C.c_int),
                ("sched", odp_schedule_param_t), ("order", C.c_int), ("nonblocking", C.c_int),
                ("context", C.c_void_p), ("context_len", C.c_uint32), ("size", C.c_uint32)]


class _qp_hash(C.Structure):
    _fields_ = [("queue_param", odp_queue_param_t), ("hash_proto", C.c_uint32)]


class _queue_union(C.Union):
    _fields_ = [("queue", C.c_void_p), ("h", _qp_hash)]


class _u64pair(C.Structure):
    _fields_ = [("max", C.c_uint64), ("min", C.c_uint64)]


class _thr_union(C.Union):
    _fields_ = [("percent", C.c_uint32 * 2), ("packet", _u64pair), ("byte", _u64pair)]


class odp_threshold_t(C.Structure):
    _anonymous_ = ("u",)
    _fields_ = [("type", C.c_int), ("u", _thr_union)]


class odp_red_param_t(C.Structure):
    _fields_ = [("enable", C.c_bool), ("threshold", odp_threshold_t)]


class odp_bp_param_t(C.Structure):
    _fields_ = [("enable", C.c_bool), ("threshold", odp_threshold_t), ("pfc_level", C.c_uint8)]


class odp_pktin_vector_config_t(C.Structure):
    _fields_ = [("enable", C.c_bool), ("pool", C.c_void_p), ("max_tmo_ns", C.c_uint64),
                ("max_size", C.c_uint32)]


class odp_cls_cos_param_t(C.Structure):
    _anonymous_ = ("u",)
    _fields_ = [("action", C.c_int), ("stats_enable", C.c_bool), ("num_queue", C.c_uint32),
                ("u", _queue_union), ("pool", C.c_void_p), ("red", odp_red_param_t),
                ("bp", odp_bp_param_t), ("vector", odp_pktin_vector_config_t)]


class odp_cls_capability_t(C.Structure):
    _fields_ = [("supported_terms", C.c_uint64), ("max_pmr", C.c_uint32),
                ("max_pmr_per_cos", C.c_uint32), ("max_terms_per_pmr", C.c_uint32),
                ("max_cos", C.c_uint32), ("max_cos_stats", C.c_uint32),
                ("max_hash_queues", C.c_uint32), ("hash_protocols", C.c_uint32),
                ("pmr_range_supported", C.c_bool), ("random_early_detection", C.c_int),
                ("threshold_red", C.c_uint8), ("back_pressure", C.c_int),
                ("threshold_bp", C.c_uint8), ("max_mark", C.c_uint64),
                ("stats_cos", C.c_uint64), ("stats_queue", C.c_uint64)]


class odp_cls_cos_stats_t(C.Structure):
    _fields_ = [("octets", C.c_uint64), ("packets", C.c_uint64), ("discards", C.c_uint64),
                ("errors", C.c_uint64)]


class odp_reass_config_t(C.Structure):
    _fields_ = [("en_ipv4", C.c_bool), ("en_ipv6", C.c_bool), ("max_wait_time", C.c_uint64),
                ("max_num_frags", C.c_uint16)]


class odp_pktio_config_t(C.Structure):
    _fields_ = [("pktin", C.c_uint64), ("pktout", C.c_uint64), ("layer", C.c_int),
                ("enable_loop", C.c_bool), ("inbound_ipsec", C.c_bool),
                ("outbound_ipsec", C.c_bool), ("enable_lso", C.c_bool),
                ("reassembly", odp_reass_config_t),
                ("pause_rx", C.c_int), ("pause_tx", C.c_int),
                ("tx_compl_modes", C.c_uint32), ("tx_compl_max_id", C.c_uint32)]


class odp_pktin_queue_param_t(C.Structure):
    _fields_ = [("op_mode", C.c_int), ("classifier_enable", C.c_bool),
                ("hash_enable", C.c_bool), ("hash_proto", C.c_uint32),
                ("num_queues", C.c_uint32), ("queue_size", C.c_uint32 * 64),
                ("queue_param", odp_queue_param_t), ("queue_param_ovr", C.c_void_p),
                ("vector", odp_pktin_vector_config_t)]


class odpg_packet_t(C.Structure):
    """include/odp_cls.h: a frame and its parse result (odpg_cls_hash_result)"""
    _fields_ = [("data", C.c_void_p), ("len", C.c_uint32), ("reserved", C.c_uint32),
                ("meta", odpg_meta_t)]


class odp_pktio_stats_t(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "in_octets", "in_packets", "in_ucast_pkts", "in_mcast_pkts", "in_bcast_pkts",
        "in_discards", "in_errors", "out_octets", "out_packets", "out_ucast_pkts",
        "out_mcast_pkts", "out_bcast_pkts", "out_discards", "out_errors")]


# ---- exported symbol table (name -> (restype, argtypes)) -------------------
_vp, _u32, _i32, _u64, _sz = C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.c_size_t
SIGNATURES = {
    # include/odpg.h
    "odpg_abi_version": (_i32, []),
    "odpg_build_info": (C.c_char_p, []),
    "odpg_device_count": (_i32, []),
    "odpg_ctx_create": (_i32, [_i32, _vp, C.POINTER(_vp)]),
    "odpg_ctx_destroy": (None, [_vp]),
    "odpg_ctx_stream": (_vp, [_vp]),
    "odpg_ctx_lanes": (_i32, [_vp]),
    "odpg_ctx_set_lanes": (_i32, [_vp, _i32]),
    "odpg_ctx_set_kernel_mode": (_i32, [_vp, _i32]),
    "odpg_last_kernel": (_i32, []),
    "odpg_ctx_sync": (_i32, [_vp]),
    "odpg_table_create": (_i32, [_vp, C.POINTER(odpg_rules_t), C.POINTER(_vp)]),
    "odpg_table_update": (_i32, [_vp, _vp, C.POINTER(odpg_rules_t)]),
    "odpg_rules_compile": (_i32, [C.POINTER(odpg_rules_t), _vp, C.POINTER(_sz)]),
    "odpg_table_import": (_i32, [_vp, _vp, _sz, C.POINTER(_vp)]),
    "odpg_table_destroy": (None, [_vp]),
    "odpg_table_num_cos": (_u32, [_vp]),
    "odpg_table_has_cycle": (_i32, [_vp]),
    "odpg_counters_create": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "odpg_counters_destroy": (None, [_vp]),
    "odpg_counters_match": (_i32, [_vp, _vp]),
    "odpg_counters_fold": (_i32, [_vp, C.POINTER(C.c_uint64)]),
    "odpg_classify": (_i32, [_vp, _vp, C.POINTER(odpg_batch_t), C.POINTER(odpg_result_t)]),
    "odpg_classify_host": (_i32, [_vp, _vp, C.POINTER(odpg_batch_t),
                                  C.POINTER(odpg_result_t), _u32]),
    "odpg_dev_alloc": (_i32, [_vp, _sz, C.POINTER(_vp)]),
    "odpg_dev_free": (_i32, [_vp, _vp]),
    "odpg_host_alloc_pinned": (_i32, [_sz, C.POINTER(_vp)]),
    "odpg_host_free_pinned": (_i32, [_vp]),
    "odpg_host_device_ptr": (_i32, [_vp, C.POINTER(_vp)]),
    "odpg_memcpy_h2d": (_i32, [_vp, _vp, _vp, _sz]),
    "odpg_memcpy_d2h": (_i32, [_vp, _vp, _vp, _sz]),
    "odpg_memset_dev": (_i32, [_vp, _vp, _i32, _sz]),
    "odpg_event_record": (_i32, [_vp, _i32]),
    "odpg_event_elapsed_ms": (_i32, [_vp, _i32, _i32, C.POINTER(C.c_float)]),
    "odpg_fence_create": (_i32, [_vp, C.POINTER(_vp)]),
    "odpg_fence_record": (_i32, [_vp, _vp]),
    "odpg_fence_query": (_i32, [_vp]),
    "odpg_fence_wait": (_i32, [_vp]),
    "odpg_fence_destroy": (None, [_vp]),
    "odpg_diag_stream": (_i32, [_vp, _vp, _u32, _vp, _i32, _u32]),
    # include/odp_cls.h
    "odp_cls_capability": (_i32, [C.POINTER(odp_cls_capability_t)]),
    "odp_cls_cos_param_init": (None, [C.POINTER(odp_cls_cos_param_t)]),
    "odp_cls_pmr_param_init": (None, [C.POINTER(odp_pmr_param_t)]),
    "odp_cls_pmr_create_opt_init": (None, [C.POINTER(odp_pmr_create_opt_t)]),
    "odp_cls_cos_create": (_vp, [C.c_char_p, C.POINTER(odp_cls_cos_param_t)]),
    "odp_cls_cos_create_multi": (_i32, [_vp, _vp, _vp, _i32]),
    "odp_cos_destroy": (_i32, [_vp]),
    "odp_cos_destroy_multi": (_i32, [C.POINTER(_vp), _i32]),
    "odp_cos_queue_set": (_i32, [_vp, _vp]),
    "odp_cos_queue": (_vp, [_vp]),
    "odp_cls_cos_num_queue": (_u32, [_vp]),
    "odp_cls_cos_queues": (_u32, [_vp, C.POINTER(_vp), _u32]),
    "odp_cls_pmr_create": (_vp, [C.POINTER(odp_pmr_param_t), _i32, _vp, _vp]),
    "odp_cls_pmr_create_opt": (_vp, [C.POINTER(odp_pmr_create_opt_t), _vp, _vp]),
    "odp_cls_pmr_create_multi": (_i32, [_vp, _vp, _vp, _vp, _i32]),
    "odp_cls_pmr_destroy": (_i32, [_vp]),
    "odp_cls_pmr_destroy_multi": (_i32, [C.POINTER(_vp), _i32]),
    "odp_cls_cos_pool_set": (_i32, [_vp, _vp]),
    "odp_cls_cos_pool": (_vp, [_vp]),
    "odp_cls_cos_stats": (_i32, [_vp, C.POINTER(odp_cls_cos_stats_t)]),
    "odp_cls_queue_stats": (_i32, [_vp, _vp, C.POINTER(odp_cls_cos_stats_t)]),
    "odp_cls_print_all": (None, []),
    "odp_cls_hash_result": (_vp, [_vp, _vp]),
    "odpg_cls_hash_result": (_vp, [_vp, C.POINTER(odpg_packet_t)]),
    "odp_queue_param_init": (None, [C.POINTER(odp_queue_param_t)]),
    "odp_pktio_param_init": (None, [_vp]),
    "odp_cos_to_u64": (_u64, [_vp]),
    "odp_pmr_to_u64": (_u64, [_vp]),
    "odp_pktio_open": (_vp, [C.c_char_p, _vp, _vp]),
    "odp_pktio_close": (_i32, [_vp]),
    "odp_pktio_config_init": (None, [C.POINTER(odp_pktio_config_t)]),
    "odp_pktio_config": (_i32, [_vp, C.POINTER(odp_pktio_config_t)]),
    "odp_pktin_queue_param_init": (None, [C.POINTER(odp_pktin_queue_param_t)]),
    "odp_pktin_queue_config": (_i32, [_vp, C.POINTER(odp_pktin_queue_param_t)]),
    "odp_pktio_start": (_i32, [_vp]),
    "odp_pktio_stop": (_i32, [_vp]),
    "odp_pktio_stats": (_i32, [_vp, C.POINTER(odp_pktio_stats_t)]),
    "odp_pktio_stats_reset": (_i32, [_vp]),
    "odp_pktio_to_u64": (_u64, [_vp]),
    "odp_pktio_default_cos_set": (_i32, [_vp, _vp]),
    "odp_pktio_error_cos_set": (_i32, [_vp, _vp]),
    "odp_pktio_skip_set": (_i32, [_vp, _u32]),
    "odp_pktio_headroom_set": (_i32, [_vp, _u32]),
    "odpg_cls_set_limits": (_i32, [_u32, _u32, _u32]),
    "odpg_cls_reset": (None, []),
    "odpg_cls_generation": (_u64, []),
    "odpg_pktio_rules": (_i32, [_vp, C.POINTER(odpg_rules_t)]),
    "odpg_pktio_recv_batch": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _i32, _vp, _vp]),
    # include/odpg_fwd.h
    "odpg_fwd_create": (_i32, [_vp, C.POINTER(odpg_route_t), _u32, C.POINTER(odpg_fwd_param_t),
                               C.POINTER(_vp)]),
    "odpg_fwd_destroy": (None, [_vp]),
    "odpg_l3fwd": (_i32, [_vp, _vp, C.POINTER(odpg_fwd_batch_t), _vp]),
    # include/odpg_pcap.h
    "odpg_pcap_read": (_i32, [C.c_char_p, _u32, C.POINTER(odpg_capture_t)]),
    "odpg_pcap_free": (None, [C.POINTER(odpg_capture_t)]),
    # include/odpg_tx.h
    "odpg_tx_prepare": (_i32, [_vp, C.POINTER(odpg_tx_batch_t), C.POINTER(odpg_tx_cfg_t), _vp]),
    # include/odpg_deliver.h
    "odpg_deliver_create": (_i32, [_vp, _vp, _u32, C.POINTER(_vp)]),
    "odpg_deliver_destroy": (None, [_vp]),
    "odpg_deliver_num_buckets": (_u32, [_vp]),
    "odpg_deliver_queue_base": (_i32, [_vp, _u32]),
    "odpg_deliver_match": (_i32, [_vp, _vp]),
    "odpg_deliver": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    # include/odpg_gather.h
    "odpg_gather_create": (_i32, [_vp, _u32, C.POINTER(_vp)]),
    "odpg_gather_destroy": (None, [_vp]),
    "odpg_gather": (_i32, [_vp, C.POINTER(odpg_gather_src_t), _vp, _vp, _u32, _u32,
                           C.POINTER(odpg_gather_dst_t)]),
    # include/odpg_lso.h
    "odpg_lso_profile_check": (_i32, [C.POINTER(odpg_lso_profile_t)]),
    "odpg_lso_create": (_i32, [_vp, C.POINTER(odpg_lso_profile_t), _u32, _u32, C.POINTER(_vp)]),
    "odpg_lso_destroy": (None, [_vp]),
    "odpg_lso": (_i32, [_vp, C.POINTER(odpg_lso_src_t), C.POINTER(odpg_lso_dst_t)]),
    # include/odpg_reass.h
    "odpg_reass_create": (_i32, [_vp, _u32, C.POINTER(_vp)]),
    "odpg_reass_destroy": (None, [_vp]),
    "odpg_reass": (_i32, [_vp, C.POINTER(odpg_reass_src_t), C.POINTER(odpg_reass_dst_t)]),
    # include/odpg_switch.h
    "odpg_switch_create": (_i32, [_vp, _u32, _u32, C.POINTER(_vp)]),
    "odpg_switch_destroy": (None, [_vp]),
    "odpg_switch_table": (_vp, [_vp]),
    "odpg_switch": (_i32, [_vp, C.POINTER(odpg_switch_src_t), C.c_uint8,
                           C.POINTER(odpg_switch_dst_t)]),
    # include/odpg_esp.h
    "odpg_esp_key_schedule": (_i32, [_vp, _u32, _vp, _vp]),
    "odpg_esp_create": (_i32, [_vp, _u32, _u32, _u32, C.POINTER(_vp)]),
    "odpg_esp_destroy": (None, [_vp]),
    "odpg_esp_sa_set": (_i32, [_vp, _u32, C.POINTER(odpg_esp_sa_t)]),
    "odpg_esp_next_seq": (_vp, [_vp]),
    "odpg_esp": (_i32, [_vp, C.POINTER(odpg_esp_src_t), C.POINTER(odpg_esp_dst_t)]),
    # include/odpg_group.h
    "odpg_group_create": (_i32, [C.POINTER(C.c_int), _u32, C.POINTER(_vp)]),
    "odpg_group_destroy": (None, [_vp]),
    "odpg_group_size": (_u32, [_vp]),
    "odpg_group_ctx": (_vp, [_vp, _u32]),
    "odpg_group_table": (_vp, [_vp, _u32]),
    "odpg_group_load": (_i32, [_vp, C.POINTER(odpg_rules_t)]),
    "odpg_group_range": (None, [_u32, _u32, _u32, C.POINTER(_u32), C.POINTER(_u32)]),
    "odpg_group_classify_host": (_i32, [_vp, C.POINTER(odpg_batch_t), C.POINTER(odpg_result_t),
                                        _i32, _u32]),
    "odpg_group_classify": (_i32, [_vp, C.POINTER(odpg_batch_t), C.POINTER(odpg_result_t),
                                   _i32]),
    "odpg_group_sync": (_i32, [_vp]),
    "odpg_group_counters_fold": (_i32, [_vp, C.POINTER(C.c_uint64)]),
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is not built: run `make -C odp_amd/csrc` or "
            "`python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            # an older experiment build (ODPG_LIB) may lack newer entry
            # points; the product library must export every one
            if os.environ.get("ODPG_LIB"):
                continue
            raise
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


class OdpgError(RuntimeError):
    pass


def check(rc, what):
    if rc != 0:
        raise OdpgError(f"{what} failed: {rc}")
    return rc
