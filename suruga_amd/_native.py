"""ctypes binding of the C ABI in ``include/suruga_gpu.h``.

The shared library is the only compute path: if it is missing or cannot be
loaded this module raises -- there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os
import threading
from pathlib import Path

from ._build import LIB

SG_OK = 0
SG_E_BAD_MAC = 1
SG_E_SHORT = 2
SG_E_ARG = -1
SG_E_HIP = -2
SG_E_NODEV = -3
SG_STATUS_SKIPPED = 3
SG_STATUS_NO_TYPE = 5

SG_BATCH_TLS = 0x1
SG_BATCH_KEEP_FAILED = 0x2
SG_KEY_LEN = 32
SG_NONCE_LEN = 8
SG_MAC_LEN = 16
SG_MAX_AD_LEN = 255
SG_MAX_RECORD_LEN = 32768
SG_MSG_MAX_LEN = 0xFFFFFFC0
SG_MSG_KEEP_FAILED = 0x1
SG_MSG_RFC8439 = 0x100
SG_RFC8439_NONCE_LEN = 12

# Every symbol include/suruga_gpu.h declares (checked by tests/test_abi.py).
EXPORTS = [
    "sg_key_size", "sg_fixed_iv_len", "sg_mac_len", "sg_abi_version",
    "sg_ctx_new", "sg_ctx_free", "sg_seal", "sg_open",
    "sg_workspace_size", "sg_seal_batch", "sg_open_batch", "sg_seal_batch_rfc8439", "sg_open_batch_rfc8439",
    "sg_seal_batch_tls13", "sg_open_batch_tls13", "sg_batch_tls13_route", "sg_seal_batch_tls13_ex", "sg_tls13_inner_len",
    "sg_fill_records", "sg_compare_records",
    "sg_last_error", "sg_build_info", "sg_source_hash", "sg_set_timing", "sg_timing_read", "sg_set_lockstep", "sg_set_packed",
    "sg_set_tls13_buckets",
    "sg_last_batch_routes",
    "sg_wire_bound", "sg_write_records", "sg_read_records", "sg_parse_records", "sg_record_timing",
    "sg_host_register", "sg_host_unregister",
    "sg_ctx_set_iv", "sg_write_records_rfc7905", "sg_read_records_rfc7905", "sg_wire_bound_tls13",
    "sg_write_records_tls13", "sg_parse_records_tls13", "sg_read_records_tls13", "sg_gather_records",
    "sg_set_record13_gather",
    "sg_sha256", "sg_hmac_sha256", "sg_prf_new", "sg_prf_get_bytes", "sg_prf_free",
    "sg_derive_keys", "sg_derive_keys_ivs", "sg_finished_verify_data",
    "sg_hkdf_extract", "sg_hkdf_expand_label", "sg_tls13_traffic_keys", "sg_tls13_traffic_keys_dev",
    "sg_ctx_set_traffic_secret", "sg_ctx_key_update",
    "sg_msg_workspace_size", "sg_seal_msg_dev", "sg_open_msg_dev", "sg_seal_msg", "sg_open_msg",
    "sg_seal_msg_rfc8439", "sg_open_msg_rfc8439",
    "sg_msg_plan_for", "sg_msg_plan_for_flags", "sg_set_msg_groups",
    "sg_msg_batch_workspace_size", "sg_seal_msg_batch", "sg_open_msg_batch", "sg_msg_batch_plan_for",
    "sg_msg_batch_plan_for_flags",
    "sg_seal_batch_quic", "sg_open_batch_quic", "sg_quic_decode_pn", "sg_quic_packet_keys",
    "sg_seal_batch_wg", "sg_open_batch_wg", "sg_wg_padded_len", "sg_wg_message_len",
    "sg_seal_batch_esp", "sg_open_batch_esp", "sg_esp_padded_len", "sg_esp_packet_len", "sg_esp_seq_hi",
    "sg_seal_batch_dtls13", "sg_open_batch_dtls13", "sg_dtls13_header_len", "sg_dtls13_inner_len", "sg_dtls13_record_len",
    "sg_dtls13_record_keys",
]
SG_MSG_BATCH_MAX_COUNT = 1 << 20
SG_MSG_MAX_GROUPS = 1024


class SgBatch(C.Structure):
    """Mirror of ``struct sg_batch``."""

    _fields_ = [
        ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("keys", C.c_void_p),
        ("num_keys", C.c_uint32),
        ("key_index", C.c_void_p),
        ("seq", C.c_void_p),
        ("seq0", C.c_uint64),
        ("content_type", C.c_uint8),
        ("ver_major", C.c_uint8),
        ("ver_minor", C.c_uint8),
        ("_pad0", C.c_uint8),
        ("nonces", C.c_void_p),
        ("ads", C.c_void_p),
        ("ad_len", C.c_uint32),
        ("ad_stride", C.c_uint32),
        ("in_", C.c_void_p),
        ("in_off", C.c_void_p),
        ("in_stride", C.c_uint64),
        ("out", C.c_void_p),
        ("out_off", C.c_void_p),
        ("out_stride", C.c_uint64),
        ("len", C.c_void_p),
        ("uniform_len", C.c_uint32),
        ("max_len", C.c_uint32),
        ("status", C.c_void_p),
        ("stream", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_size", C.c_size_t),
    ]


class SgBatchRfc8439(C.Structure):
    """Mirror of ``struct sg_batch_rfc8439``."""

    _fields_ = [("ivs", C.c_void_p), ("flags", C.c_uint32), ("_pad", C.c_uint32)]


class SgBatchTls13(C.Structure):
    """Mirror of ``struct sg_batch_tls13``."""

    _fields_ = [("ivs", C.c_void_p), ("inner_type", C.c_void_p), ("content_len", C.c_void_p), ("flags", C.c_uint32),
                ("_pad", C.c_uint32)]


class SgTls13SealOpts(C.Structure):
    """Mirror of ``struct sg_tls13_seal_opts``."""

    _fields_ = [("inner_types", C.c_void_p), ("pad_to", C.c_uint32), ("flags", C.c_uint32)]


SG_TLS13_MAX_INNER = (1 << 14) + 1
SG_TLS13_KEYS_UPDATE = 0x1


class SgTls13Keys(C.Structure):
    """Mirror of ``struct sg_tls13_keys``."""

    _fields_ = [("count", C.c_uint32), ("flags", C.c_uint32), ("rows", C.c_uint32), ("_pad", C.c_uint32),
                ("index", C.c_void_p), ("secrets", C.c_void_p), ("keys", C.c_void_p), ("ivs", C.c_void_p),
                ("stream", C.c_void_p)]


SG_QUIC_MAX_PACKET_LEN = 16384
SG_QUIC_MAX_PN_OFF = 251
SG_QUIC_KEY_PHASE = 0x1
SG_QUIC_KEEP_FAILED = 0x2


class SgQuicBatch(C.Structure):
    """Mirror of ``struct sg_quic_batch``."""

    _fields_ = [
        ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("keys", C.c_void_p),
        ("ivs", C.c_void_p),
        ("hp_keys", C.c_void_p),
        ("key_index", C.c_void_p),
        ("pn", C.c_void_p),
        ("pn_out", C.c_void_p),
        ("pn_off", C.c_void_p),
        ("num_keys", C.c_uint32),
        ("uniform_pn_off", C.c_uint32),
        ("in_", C.c_void_p),
        ("in_off", C.c_void_p),
        ("in_stride", C.c_uint64),
        ("out", C.c_void_p),
        ("out_off", C.c_void_p),
        ("out_stride", C.c_uint64),
        ("len", C.c_void_p),
        ("uniform_len", C.c_uint32),
        ("max_len", C.c_uint32),
        ("status", C.c_void_p),
        ("stream", C.c_void_p),
    ]


SG_WG_HEADER_LEN = 16
SG_WG_MAX_MESSAGE_LEN = 16384
SG_WG_KEEP_FAILED = 0x1
SG_STATUS_BAD_HEADER = 6
SG_STATUS_BAD_INNER = 7


class SgWgBatch(C.Structure):
    """Mirror of ``struct sg_wg_batch``."""

    _fields_ = [
        ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("keys", C.c_void_p),
        ("receiver", C.c_void_p),
        ("key_index", C.c_void_p),
        ("counter", C.c_void_p),
        ("counter_out", C.c_void_p),
        ("inner_len", C.c_void_p),
        ("num_keys", C.c_uint32),
        ("pad_cap", C.c_uint32),
        ("in_", C.c_void_p),
        ("in_off", C.c_void_p),
        ("in_stride", C.c_uint64),
        ("out", C.c_void_p),
        ("out_off", C.c_void_p),
        ("out_stride", C.c_uint64),
        ("len", C.c_void_p),
        ("uniform_len", C.c_uint32),
        ("max_len", C.c_uint32),
        ("status", C.c_void_p),
        ("stream", C.c_void_p),
    ]


SG_ESP_HEADER_LEN = 16
SG_ESP_MAX_PACKET_LEN = 16384
SG_ESP_ESN = 0x1
SG_ESP_KEEP_FAILED = 0x2


class SgEspBatch(C.Structure):
    """Mirror of ``struct sg_esp_batch``."""

    _fields_ = [
        ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("keys", C.c_void_p),
        ("salts", C.c_void_p),
        ("spi", C.c_void_p),
        ("sa_index", C.c_void_p),
        ("seq", C.c_void_p),
        ("iv", C.c_void_p),
        ("next_header", C.c_void_p),
        ("seq_out", C.c_void_p),
        ("payload_len", C.c_void_p),
        ("next_header_out", C.c_void_p),
        ("replay_top", C.c_void_p),
        ("num_sas", C.c_uint32),
        ("align", C.c_uint32),
        ("uniform_next_header", C.c_uint32),
        ("window", C.c_uint32),
        ("in_", C.c_void_p),
        ("in_off", C.c_void_p),
        ("in_stride", C.c_uint64),
        ("out", C.c_void_p),
        ("out_off", C.c_void_p),
        ("out_stride", C.c_uint64),
        ("len", C.c_void_p),
        ("uniform_len", C.c_uint32),
        ("max_len", C.c_uint32),
        ("status", C.c_void_p),
        ("stream", C.c_void_p),
    ]


SG_DTLS13_MAX_CONTENT_LEN = 16384
SG_DTLS13_MAX_CID_LEN = 250
SG_DTLS13_MAX_RECORD_LEN = 255 + 16384 + 1 + 16
SG_DTLS13_SEQ16 = 0x1
SG_DTLS13_LENGTH = 0x2
SG_DTLS13_EPOCH_ROWS = 0x4
SG_DTLS13_KEEP_FAILED = 0x8


class SgDtls13Batch(C.Structure):
    """Mirror of ``struct sg_dtls13_batch``."""

    _fields_ = [
        ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("keys", C.c_void_p),
        ("ivs", C.c_void_p),
        ("sn_keys", C.c_void_p),
        ("cids", C.c_void_p),
        ("key_index", C.c_void_p),
        ("seq", C.c_void_p),
        ("type", C.c_void_p),
        ("epoch", C.c_void_p),
        ("expected", C.c_void_p),
        ("seq_out", C.c_void_p),
        ("epoch_out", C.c_void_p),
        ("content_len", C.c_void_p),
        ("type_out", C.c_void_p),
        ("num_conns", C.c_uint32),
        ("cid_len", C.c_uint32),
        ("pad_to", C.c_uint32),
        ("uniform_type", C.c_uint8),
        ("uniform_epoch", C.c_uint8),
        ("in_", C.c_void_p),
        ("in_off", C.c_void_p),
        ("in_stride", C.c_uint64),
        ("out", C.c_void_p),
        ("out_off", C.c_void_p),
        ("out_stride", C.c_uint64),
        ("len", C.c_void_p),
        ("uniform_len", C.c_uint32),
        ("max_len", C.c_uint32),
        ("status", C.c_void_p),
        ("stream", C.c_void_p),
    ]


class SgBatchRoutes(C.Structure):
    """Mirror of ``struct sg_batch_routes``."""

    _fields_ = [("known", C.c_uint32), ("classes", C.c_uint32), ("bucket", C.c_uint32 * 3), ("packed", C.c_uint32),
                ("skipped", C.c_uint32), ("_pad", C.c_uint32)]


class SgMsg(C.Structure):
    """Mirror of ``struct sg_msg``."""

    _fields_ = [
        ("key", C.c_void_p),
        ("nonce", C.c_uint8 * 8),
        ("ad", C.c_void_p),
        ("ad_len", C.c_uint64),
        ("in_", C.c_void_p),
        ("in_len", C.c_uint64),
        ("out", C.c_void_p),
        ("status", C.c_void_p),
        ("flags", C.c_uint32),
        ("nonce_hi", C.c_uint8 * 4),  # SG_MSG_RFC8439 only; the struct's former padding
        ("stream", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_size", C.c_size_t),
    ]


class SgMsgPlan(C.Structure):
    """Mirror of ``struct sg_msg_plan``."""

    _fields_ = [("mac_blocks", C.c_uint64), ("tiles", C.c_uint64), ("zero_blocks", C.c_uint64),
                ("tile_blocks", C.c_uint32), ("tile_bytes", C.c_uint32), ("groups", C.c_uint32),
                ("tiles_per_group", C.c_uint32)]


class SgMsgItem(C.Structure):
    """Mirror of ``struct sg_msg_item``."""

    _fields_ = [
        ("key_index", C.c_uint32),
        ("nonce", C.c_uint8 * 8),
        ("nonce_hi", C.c_uint8 * 4),  # SG_MSG_RFC8439 only; the struct's former padding
        ("ad", C.c_void_p),
        ("ad_len", C.c_uint64),
        ("in_", C.c_void_p),
        ("in_len", C.c_uint64),
        ("out", C.c_void_p),
    ]


class SgMsgBatch(C.Structure):
    """Mirror of ``struct sg_msg_batch``."""

    _fields_ = [
        ("count", C.c_uint32),
        ("flags", C.c_uint32),
        ("keys", C.c_void_p),
        ("num_keys", C.c_uint32),
        ("items", C.POINTER(SgMsgItem)),
        ("status", C.c_void_p),
        ("stream", C.c_void_p),
        ("workspace", C.c_void_p),
        ("workspace_size", C.c_size_t),
    ]


class SgMsgSeg(C.Structure):
    """Mirror of ``struct sg_msg_seg``."""

    _fields_ = [("msg", C.c_uint32), ("tile_begin", C.c_uint32), ("tile_end", C.c_uint32), ("group", C.c_uint32)]


class SgMsgSpan(C.Structure):
    """Mirror of ``struct sg_msg_span``."""

    _fields_ = [("first", C.c_uint32), ("count", C.c_uint32)]


class SgMsgBatchPlan(C.Structure):
    """Mirror of ``struct sg_msg_batch_plan``."""

    _fields_ = [("tiles", C.c_uint64), ("tiles_per_group", C.c_uint64), ("groups", C.c_uint32),
                ("segments", C.c_uint32), ("tile_blocks", C.c_uint32), ("tile_bytes", C.c_uint32)]


class SgReadResult(C.Structure):
    """Mirror of ``struct sg_read_result``."""

    _fields_ = [("records", C.c_uint64), ("consumed", C.c_uint64), ("out_len", C.c_uint64),
                ("error", C.c_int32), ("_pad", C.c_uint32)]


class SgGatherCursor(C.Structure):
    """Mirror of ``struct sg_gather_cursor``."""

    _fields_ = [("offset", C.c_uint64), ("stopped", C.c_uint32), ("_pad", C.c_uint32)]


class SgWireRecord(C.Structure):
    """Mirror of ``struct sg_wire_record``."""

    _fields_ = [("offset", C.c_uint64), ("frag_len", C.c_uint32), ("type", C.c_uint8), ("ver_major", C.c_uint8),
                ("ver_minor", C.c_uint8), ("_pad", C.c_uint8)]


SG_E_UNEXPECTED_MESSAGE = 3
SG_E_RECORD_OVERFLOW = 4
SG_RECORD_MAX_LEN = 16384
SG_ENC_RECORD_MAX_LEN = 16384 + 2048
SG_HEADER_LEN = 5


class NativeError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"suruga_gpu error {code}: {msg}")
        self.code = code


_lib = None
_lock = threading.Lock()


def provenance_error(got: str, want: str, allow_variant: bool):
    """None when a library embedding source marker `got` may run in a tree
    whose sources hash to `want`, else the reason.  Experiment variants
    (tools/build_variant.py, _build.build_library(defines=...)) embed
    "<tree hash>+var:<name>:<edit hash>" and run only on explicit request
    (SURUGA_ALLOW_VARIANT=1, as tools/ab_libs.sh sets).  allow_variant ==
    "foreign" (SURUGA_ALLOW_VARIANT=foreign) also admits a variant built from an
    earlier tree -- the A/B of a change against the build before it
    (tools/build_variant.py with no edits) -- and nothing unmarked."""
    if got == want:
        return None
    if allow_variant == "foreign" and "+var:" in got:
        return None
    if got.startswith(want + "+var:"):
        if allow_variant:
            return None
        return (f"is an experiment variant ({got}) of this tree: set SURUGA_ALLOW_VARIANT=1 to time it; "
                "the product runs only the tree's own build")
    return (f"was built from other sources (embedded hash {got}, tree {want}): "
            "rebuild with `python -m suruga_amd._build`")


def _declare(lib: C.CDLL) -> None:
    u8p = C.POINTER(C.c_uint8)
    lib.sg_key_size.restype = C.c_size_t
    lib.sg_fixed_iv_len.restype = C.c_size_t
    lib.sg_mac_len.restype = C.c_size_t
    lib.sg_abi_version.restype = C.c_int
    lib.sg_ctx_new.restype = C.c_void_p
    lib.sg_ctx_new.argtypes = [C.c_char_p, C.c_int]
    lib.sg_ctx_free.restype = None
    lib.sg_ctx_free.argtypes = [C.c_void_p]
    for f in (lib.sg_seal, lib.sg_open):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                      C.c_char_p, C.c_size_t, u8p]
    lib.sg_workspace_size.restype = C.c_size_t
    lib.sg_workspace_size.argtypes = [C.c_uint32]
    for f in (lib.sg_seal_batch, lib.sg_open_batch):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgBatch)]
    for f in (lib.sg_seal_batch_rfc8439, lib.sg_open_batch_rfc8439):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgBatch), C.POINTER(SgBatchRfc8439)]
    for f in (lib.sg_seal_batch_tls13, lib.sg_open_batch_tls13):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgBatch), C.POINTER(SgBatchTls13)]
    lib.sg_seal_batch_tls13_ex.restype = C.c_int
    lib.sg_seal_batch_tls13_ex.argtypes = [C.POINTER(SgBatch), C.POINTER(SgBatchTls13), C.POINTER(SgTls13SealOpts)]
    lib.sg_tls13_inner_len.restype = C.c_uint32
    lib.sg_tls13_inner_len.argtypes = [C.c_uint32, C.c_uint32]
    lib.sg_batch_tls13_route.restype = C.c_int
    lib.sg_batch_tls13_route.argtypes = [C.POINTER(SgBatch), C.c_int]
    lib.sg_fill_records.restype = C.c_int
    lib.sg_fill_records.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint64,
                                    C.c_uint64, C.c_void_p]
    lib.sg_compare_records.restype = C.c_int
    lib.sg_compare_records.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32,
                                       C.c_uint32, C.c_void_p, C.c_void_p]
    lib.sg_last_error.restype = C.c_char_p
    lib.sg_build_info.restype = C.c_char_p
    lib.sg_source_hash.restype = C.c_char_p
    lib.sg_set_timing.restype = C.c_int
    lib.sg_set_timing.argtypes = [C.c_int]
    lib.sg_set_lockstep.restype = C.c_int
    lib.sg_set_lockstep.argtypes = [C.c_int]
    lib.sg_set_packed.restype = C.c_int
    lib.sg_set_packed.argtypes = [C.c_int]
    lib.sg_set_tls13_buckets.restype = C.c_int
    lib.sg_set_tls13_buckets.argtypes = [C.c_int]
    lib.sg_last_batch_routes.restype = C.c_int
    lib.sg_last_batch_routes.argtypes = [C.POINTER(SgBatchRoutes)]
    lib.sg_timing_read.restype = C.c_int
    d = C.POINTER(C.c_double)
    u = C.POINTER(C.c_uint32)
    lib.sg_timing_read.argtypes = [d, d, d, u, u, u]
    lib.sg_wire_bound.restype = C.c_size_t
    lib.sg_wire_bound.argtypes = [C.c_size_t]
    lib.sg_write_records.restype = C.c_int64
    lib.sg_write_records.argtypes = [C.c_void_p, C.c_uint64, C.c_uint8, C.c_uint8, C.c_uint8, C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    lib.sg_read_records.restype = C.c_int
    lib.sg_read_records.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                    C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(SgReadResult)]
    lib.sg_host_register.restype = C.c_int
    lib.sg_host_register.argtypes = [C.c_void_p, C.c_size_t]
    lib.sg_host_unregister.restype = C.c_int
    lib.sg_host_unregister.argtypes = [C.c_void_p]
    lib.sg_parse_records.restype = C.c_int
    lib.sg_parse_records.argtypes = [C.c_void_p, C.c_size_t, C.c_size_t, C.POINTER(SgWireRecord),
                                     C.POINTER(C.c_size_t), C.POINTER(C.c_int32)]
    lib.sg_record_timing.restype = C.c_int
    lib.sg_record_timing.argtypes = [d, d, d, d]
    lib.sg_ctx_set_iv.restype = C.c_int
    lib.sg_ctx_set_iv.argtypes = [C.c_void_p, C.c_char_p]
    lib.sg_write_records_rfc7905.restype = C.c_int64
    lib.sg_write_records_rfc7905.argtypes = lib.sg_write_records.argtypes
    lib.sg_wire_bound_tls13.restype = C.c_size_t
    lib.sg_wire_bound_tls13.argtypes = [C.c_size_t]
    lib.sg_write_records_tls13.restype = C.c_int64
    lib.sg_write_records_tls13.argtypes = [C.c_void_p, C.c_uint64, C.c_uint8, C.c_void_p, C.c_size_t, C.c_void_p,
                                           C.c_size_t, C.POINTER(C.c_size_t)]
    for f in (lib.sg_read_records_rfc7905, lib.sg_read_records_tls13):
        f.restype = C.c_int
        f.argtypes = lib.sg_read_records.argtypes
    lib.sg_parse_records_tls13.restype = C.c_int
    lib.sg_parse_records_tls13.argtypes = lib.sg_parse_records.argtypes
    lib.sg_gather_records.restype = C.c_int
    lib.sg_gather_records.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.sg_set_record13_gather.restype = C.c_int
    lib.sg_set_record13_gather.argtypes = [C.c_int]
    vp = C.c_void_p
    lib.sg_sha256.restype = None
    lib.sg_sha256.argtypes = [vp, C.c_size_t, vp]
    lib.sg_hmac_sha256.restype = C.c_int
    lib.sg_hmac_sha256.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.sg_prf_new.restype = vp
    lib.sg_prf_new.argtypes = [vp, C.c_size_t, vp, C.c_size_t]
    lib.sg_prf_get_bytes.restype = C.c_int
    lib.sg_prf_get_bytes.argtypes = [vp, vp, C.c_size_t]
    lib.sg_prf_free.restype = None
    lib.sg_prf_free.argtypes = [vp]
    lib.sg_derive_keys.restype = C.c_int
    lib.sg_derive_keys.argtypes = [C.c_uint32, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, C.c_int]
    lib.sg_derive_keys_ivs.restype = C.c_int
    lib.sg_derive_keys_ivs.argtypes = [C.c_uint32, vp, C.c_size_t, C.c_size_t, vp, vp, vp, vp, vp, vp, vp, C.c_int]
    lib.sg_finished_verify_data.restype = C.c_int
    lib.sg_finished_verify_data.argtypes = [vp, C.c_int, vp, vp]
    lib.sg_hkdf_extract.restype = C.c_int
    lib.sg_hkdf_extract.argtypes = [vp, C.c_size_t, vp, C.c_size_t, vp]
    lib.sg_hkdf_expand_label.restype = C.c_int
    lib.sg_hkdf_expand_label.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_size_t]
    lib.sg_tls13_traffic_keys.restype = C.c_int
    lib.sg_tls13_traffic_keys.argtypes = [C.c_uint32, vp, vp, vp, C.c_int, C.c_int]
    lib.sg_tls13_traffic_keys_dev.restype = C.c_int
    lib.sg_tls13_traffic_keys_dev.argtypes = [C.POINTER(SgTls13Keys)]
    for f in (lib.sg_seal_batch_quic, lib.sg_open_batch_quic):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgQuicBatch)]
    lib.sg_quic_decode_pn.restype = C.c_uint64
    lib.sg_quic_decode_pn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    lib.sg_quic_packet_keys.restype = C.c_int
    lib.sg_quic_packet_keys.argtypes = [C.c_uint32, vp, vp, vp, vp, C.c_int, C.c_int]
    for f in (lib.sg_seal_batch_wg, lib.sg_open_batch_wg):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgWgBatch)]
    for f in (lib.sg_wg_padded_len, lib.sg_wg_message_len):
        f.restype = C.c_uint32
        f.argtypes = [C.c_uint32, C.c_uint32]
    for f in (lib.sg_seal_batch_esp, lib.sg_open_batch_esp):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgEspBatch)]
    for f in (lib.sg_esp_padded_len, lib.sg_esp_packet_len):
        f.restype = C.c_uint32
        f.argtypes = [C.c_uint32, C.c_uint32]
    lib.sg_esp_seq_hi.restype = C.c_uint32
    lib.sg_esp_seq_hi.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
    for f in (lib.sg_seal_batch_dtls13, lib.sg_open_batch_dtls13):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgDtls13Batch)]
    lib.sg_dtls13_header_len.restype = C.c_uint32
    lib.sg_dtls13_header_len.argtypes = [C.c_uint32, C.c_uint32]
    lib.sg_dtls13_inner_len.restype = C.c_uint32
    lib.sg_dtls13_inner_len.argtypes = [C.c_uint32, C.c_uint32]
    lib.sg_dtls13_record_len.restype = C.c_uint32
    lib.sg_dtls13_record_len.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]
    lib.sg_dtls13_record_keys.restype = C.c_int
    lib.sg_dtls13_record_keys.argtypes = [C.c_uint32, vp, vp, vp, vp, C.c_int, C.c_int]
    lib.sg_ctx_set_traffic_secret.restype = C.c_int
    lib.sg_ctx_set_traffic_secret.argtypes = [C.c_void_p, C.c_char_p]
    lib.sg_ctx_key_update.restype = C.c_int
    lib.sg_ctx_key_update.argtypes = [C.c_void_p]
    lib.sg_msg_workspace_size.restype = C.c_size_t
    lib.sg_msg_workspace_size.argtypes = []
    for f in (lib.sg_seal_msg_dev, lib.sg_open_msg_dev):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgMsg)]
    for f in (lib.sg_seal_msg, lib.sg_open_msg, lib.sg_seal_msg_rfc8439, lib.sg_open_msg_rfc8439):
        f.restype = C.c_int
        f.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t,
                      C.c_char_p, C.c_size_t, u8p]
    lib.sg_msg_plan_for.restype = C.c_int
    lib.sg_msg_plan_for.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(SgMsgPlan)]
    lib.sg_msg_plan_for_flags.restype = C.c_int
    lib.sg_msg_plan_for_flags.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(SgMsgPlan)]
    lib.sg_set_msg_groups.restype = C.c_int
    lib.sg_set_msg_groups.argtypes = [C.c_int]
    lib.sg_msg_batch_workspace_size.restype = C.c_size_t
    lib.sg_msg_batch_workspace_size.argtypes = [C.c_uint32]
    for f in (lib.sg_seal_msg_batch, lib.sg_open_msg_batch):
        f.restype = C.c_int
        f.argtypes = [C.POINTER(SgMsgBatch)]
    u64p = C.POINTER(C.c_uint64)
    lib.sg_msg_batch_plan_for.restype = C.c_int
    lib.sg_msg_batch_plan_for.argtypes = [u64p, u64p, C.c_uint32, C.c_uint32, C.POINTER(SgMsgBatchPlan),
                                          C.POINTER(SgMsgPlan), C.POINTER(SgMsgSeg), C.c_uint32,
                                          C.POINTER(SgMsgSpan), C.POINTER(SgMsgSpan)]
    lib.sg_msg_batch_plan_for_flags.restype = C.c_int
    lib.sg_msg_batch_plan_for_flags.argtypes = [u64p, u64p, C.c_uint32, C.c_uint32, C.c_uint32,
                                                C.POINTER(SgMsgBatchPlan), C.POINTER(SgMsgPlan), C.POINTER(SgMsgSeg),
                                                C.c_uint32, C.POINTER(SgMsgSpan), C.POINTER(SgMsgSpan)]


def load(path: Path | None = None) -> C.CDLL:
    """Load (once) and return the native library.  Raises if it is missing."""
    global _lib
    with _lock:
        if _lib is None:
            # SURUGA_GPU_LIB: load another build of the same library (A/B kernel
            # experiments, tools/ab_bench.sh); still the HIP library, never a fallback
            p = Path(path or os.environ.get("SURUGA_GPU_LIB") or LIB)
            if not p.exists():
                raise ImportError(
                    f"{p} is missing: build it with `python -m suruga_amd._build` "
                    "(hipcc --offload-arch=gfx950); there is no CPU fallback")
            lib = C.CDLL(str(p))
            _declare(lib)
            # provenance: the library must have been built from this tree's
            # sources (a stale prebuilt .so whose file time happens to be newer
            # would otherwise run silently)
            from ._build import source_hash

            got, want = lib.sg_source_hash().decode(), source_hash()
            av = os.environ.get("SURUGA_ALLOW_VARIANT")
            err = provenance_error(got, want, "foreign" if av == "foreign" else av == "1")
            if err:
                raise ImportError(f"{p} {err}")
            global _lib_path
            _lib_path = str(p.resolve())
            _lib = lib
        return _lib


_lib_path = None


def loaded_info() -> dict:
    """Which library this process runs and the source hash it carries (bench provenance)."""
    lib = load()
    return {"path": _lib_path, "source_hash": lib.sg_source_hash().decode()}


def last_error() -> str:
    return load().sg_last_error().decode(errors="replace")


def check(code: int) -> int:
    """Raise NativeError for negative (argument / runtime) codes."""
    if code < 0:
        raise NativeError(code, last_error())
    return code
