"""Device-resident batch seal/open (``sg_seal_batch`` / ``sg_open_batch``).

This is the batched form of the record layer's hot loop: ``TlsWriter``'s
``write_data`` chunk loop (tls.rs:137-147 -> write_record tls.rs:99-135) and
``TlsReader::read_record`` (tls.rs:217-281).  In TLS mode the nonce
(``u64_be_array(seq)``, tls.rs:103) and the 13-byte additional data
(tls.rs:105-112 / 250-265) are built on the device from the sequence number,
so a call carries only record bytes, lengths and keys.

With ``rfc8439=True`` the same batch runs through ``sg_seal_batch_rfc8439`` /
``sg_open_batch_rfc8439``: RFC 8439 with 12-byte nonces, and in TLS mode the
RFC 7905 nonce (the key's write IV in ``ivs`` XOR the sequence number).

``seal_tls13`` / ``open_tls13`` run it as TLS 1.3 records (RFC 8446 section 5.2,
``sg_seal_batch_tls13`` / ``sg_open_batch_tls13``): the device appends the
inner type byte on seal and returns ``inner_type`` / ``content_len`` on open;
``seal_tls13(batch, pad_to=, inner_types=)`` pads the records (RFC 8446 section 5.4)
and takes a type per record (``sg_seal_batch_tls13_ex``).

Tensors are torch tensors on the GPU (PyTorch is used here only for device
memory and streams); all arithmetic runs in the gfx950 kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

from . import _native as N

APPLICATION_DATA = 23  # ContentType::ApplicationDataTy (tls.rs:26)
TLS_VERSION = (3, 3)   # tls.rs:17


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    return int(t.data_ptr())


def _stream_handle(stream) -> Optional[int]:
    if stream is None:
        import torch

        return int(torch.cuda.current_stream().cuda_stream)
    if isinstance(stream, int):
        return stream
    return int(stream.cuda_stream)


@dataclass
class Batch:
    """Arguments of one ``sg_*_batch`` call (see include/suruga_gpu.h)."""

    count: int
    keys: object                      # uint8 [num_keys, 32], device
    inp: object                       # uint8 device buffer
    out: object                       # uint8 device buffer
    uniform_len: int = 0
    lens: object = None               # uint32 [count] device, or None
    max_len: int = 0
    in_stride: int = 0
    out_stride: int = 0
    in_off: object = None             # uint64 [count] device, or None
    out_off: object = None
    key_index: object = None          # uint32 [count] device, or None
    tls: bool = True
    seq0: int = 0
    seq: object = None                # uint64 [count] device, or None
    content_type: int = APPLICATION_DATA
    version: tuple = TLS_VERSION
    nonces: object = None             # explicit mode: uint8 [count, 8]
    ads: object = None                # explicit mode: uint8 [count, ad_stride]
    ad_len: int = 0
    ad_stride: int = 0
    status: object = None             # uint8 [count] device (open)
    workspace: object = None          # uint8 [>= workspace_size(count)] device, or None
    stream: object = None             # torch.cuda.Stream / raw handle (0: the NULL stream) / None = current stream
    keep_failed: bool = False         # open: keep the unauthenticated plaintext of BAD_MAC records
    rfc8439: bool = False             # RFC 8439 / RFC 7905 (explicit mode: nonces are uint8 [count, 12])
    ivs: object = None                # rfc8439 TLS mode / TLS 1.3: uint8 [num_keys, 12] device, the write IVs
    inner_type: object = None         # open_tls13: uint8 [count] device, the records' inner content types
    content_len: object = None        # open_tls13: uint32 [count] device, the records' content lengths

    def to_c_tls13(self) -> N.SgBatchTls13:
        x = N.SgBatchTls13()
        x.ivs = _ptr(self.ivs)
        x.inner_type = _ptr(self.inner_type)
        x.content_len = _ptr(self.content_len)
        x.flags = 0
        return x

    def to_c_rfc8439(self) -> N.SgBatchRfc8439:
        x = N.SgBatchRfc8439()
        x.ivs = _ptr(self.ivs)
        x.flags = 0
        return x

    def to_c(self) -> N.SgBatch:
        b = N.SgBatch()
        b.count = self.count
        b.flags = (N.SG_BATCH_TLS if self.tls else 0) | (N.SG_BATCH_KEEP_FAILED if self.keep_failed else 0)
        b.keys = _ptr(self.keys)
        b.num_keys = int(self.keys.shape[0]) if hasattr(self.keys, "shape") and self.keys.dim() == 2 else max(
            1, int(self.keys.numel()) // 32)
        b.key_index = _ptr(self.key_index)
        b.seq = _ptr(self.seq)
        b.seq0 = self.seq0 & 0xFFFFFFFFFFFFFFFF
        b.content_type = self.content_type
        b.ver_major, b.ver_minor = self.version
        b.nonces = _ptr(self.nonces)
        b.ads = _ptr(self.ads)
        b.ad_len = self.ad_len
        b.ad_stride = self.ad_stride
        b.in_ = _ptr(self.inp)
        b.in_off = _ptr(self.in_off)
        b.in_stride = self.in_stride
        b.out = _ptr(self.out)
        b.out_off = _ptr(self.out_off)
        b.out_stride = self.out_stride
        b.len = _ptr(self.lens)
        b.uniform_len = self.uniform_len
        b.max_len = self.max_len
        b.status = _ptr(self.status)
        b.stream = _stream_handle(self.stream)
        b.workspace = _ptr(self.workspace)
        b.workspace_size = int(self.workspace.numel()) if self.workspace is not None else 0
        return b


def workspace_size(count: int) -> int:
    return int(N.load().sg_workspace_size(count))


def seal(batch: Batch) -> None:
    """Seal every record: out_i = ct_i || tag_i (chacha20_poly1305.rs:48-59)."""
    cb = batch.to_c()
    if batch.rfc8439:
        xb = batch.to_c_rfc8439()
        N.check(N.load().sg_seal_batch_rfc8439(C.byref(cb), C.byref(xb)))
        return
    if batch.ivs is not None:
        raise ValueError("ivs belong to rfc8439=True")
    N.check(N.load().sg_seal_batch(C.byref(cb)))


def open_(batch: Batch) -> None:
    """Open every record; per-record status lands in ``batch.status``
    (0 ok, 1 BadRecordMac "wrong mac", 2 BadRecordMac "message too short")."""
    if batch.status is None:
        raise ValueError("open needs a status tensor")
    cb = batch.to_c()
    if batch.rfc8439:
        xb = batch.to_c_rfc8439()
        N.check(N.load().sg_open_batch_rfc8439(C.byref(cb), C.byref(xb)))
        return
    if batch.ivs is not None:
        raise ValueError("ivs belong to rfc8439=True")
    N.check(N.load().sg_open_batch(C.byref(cb)))


def seal_tls13(batch: Batch, pad_to: int = 0, inner_types=None) -> None:
    """Seal every record as a TLS 1.3 record: out_i = ct(content_i || type_i || zeros) || tag_i,
    ``tls13_inner_len(len_i, pad_to) + 16`` bytes (RFC 8446 section 5.2, 5.4).  The type is
    ``batch.content_type``, or ``inner_types[i]`` (uint8 [count], device) where given.  Without
    ``pad_to`` and ``inner_types`` this is ``sg_seal_batch_tls13`` (len_i + 17 bytes), otherwise
    ``sg_seal_batch_tls13_ex``."""
    cb, xb = batch.to_c(), batch.to_c_tls13()
    if not pad_to and inner_types is None:
        N.check(N.load().sg_seal_batch_tls13(C.byref(cb), C.byref(xb)))
        return
    o = N.SgTls13SealOpts()
    o.inner_types, o.pad_to, o.flags = _ptr(inner_types), pad_to, 0
    N.check(N.load().sg_seal_batch_tls13_ex(C.byref(cb), C.byref(xb), C.byref(o)))


def tls13_inner_len(n: int, pad_to: int) -> int:
    """Length of the inner plaintext a TLS 1.3 seal builds of ``n`` content bytes under ``pad_to``
    (``sg_tls13_inner_len``): n + 1, rounded up to a multiple of pad_to, at most 2^14 + 1."""
    return int(N.load().sg_tls13_inner_len(n, pad_to))


def open_tls13(batch: Batch) -> None:
    """Open every TLS 1.3 record: the inner plaintext lands in ``out``, the status in
    ``batch.status`` (0 ok, 1 wrong mac, 2 too short, 5 no inner type), and for status 0
    the inner type and the content length in ``batch.inner_type`` / ``batch.content_len``."""
    if batch.status is None or batch.inner_type is None or batch.content_len is None:
        raise ValueError("open_tls13 needs status, inner_type and content_len tensors")
    cb, xb = batch.to_c(), batch.to_c_tls13()
    N.check(N.load().sg_open_batch_tls13(C.byref(cb), C.byref(xb)))


def tls13_route(batch: Batch, open: bool) -> int:  # noqa: A002  (the C argument's name)
    """The route ``seal_tls13`` / ``open_tls13`` would take, without any GPU call: 1 the uniform
    wave-per-record kernel, 0 not that route -- the size classes and, for the eligible records
    of a mixed batch, the packed kernel, which ``last_routes`` reports (``sg_batch_tls13_route``)."""
    cb = batch.to_c()
    return N.check(N.load().sg_batch_tls13_route(C.byref(cb), 1 if open else 0))


def set_tls13_buckets(enable: int) -> int:
    """``sg_set_tls13_buckets``: 1 routes the padded TLS 1.3 records of 4-16 KiB inner length of a
    mixed batch to the wave-per-record buckets, 0 (the default) to the size classes; negative only
    queries.  Returns the previous setting."""
    return int(N.load().sg_set_tls13_buckets(enable))


def fill_records(buf, stride: int, length: int, count: int, seed: int, j0: int = 0, stream=None) -> None:
    """Synthetic records generated on the device (splitmix64 rule)."""
    N.check(N.load().sg_fill_records(_ptr(buf), stride, length, count, seed & (2**64 - 1), j0,
                                     _stream_handle(stream)))


def compare_records(a, stride_a: int, b, stride_b: int, length: int, count: int, mismatches,
                    stream=None) -> None:
    N.check(N.load().sg_compare_records(_ptr(a), stride_a, _ptr(b), stride_b, length, count,
                                        _ptr(mismatches), _stream_handle(stream)))


def set_timing(enable: bool) -> None:
    N.check(N.load().sg_set_timing(1 if enable else 0))


def timing_read() -> dict:
    d = [C.c_double() for _ in range(3)]
    u = [C.c_uint32() for _ in range(3)]
    N.check(N.load().sg_timing_read(C.byref(d[0]), C.byref(d[1]), C.byref(d[2]), C.byref(u[0]),
                                    C.byref(u[1]), C.byref(u[2])))
    return {"seal_ms": d[0].value, "open_ms": d[1].value, "keying_ms": d[2].value,
            "n_seal": u[0].value, "n_open": u[1].value, "n_keying": u[2].value}


def last_routes() -> dict:
    """Where the records of this thread's last ``seal`` / ``open_`` / ``seal_tls13`` / ``open_tls13`` went
    (``sg_last_batch_routes``): ``known`` is False unless that call was a mixed
    batch whose list populations the dispatcher read back."""
    r = N.SgBatchRoutes()
    N.check(N.load().sg_last_batch_routes(C.byref(r)))
    return {"known": bool(r.known), "classes": int(r.classes), "bucket": [int(x) for x in r.bucket],
            "packed": int(r.packed), "skipped": int(r.skipped)}
