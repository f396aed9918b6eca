"""CPU tests of the RFC 8439 record batch's C boundary (sg_seal_batch_rfc8439 /
sg_open_batch_rfc8439, include/suruga_gpu.h): the extension struct's layout and
every rejection, all made before any GPU call (there is no GPU here)."""
from __future__ import annotations

import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def tls_batch():
    from suruga_amd._native import SG_BATCH_TLS, SgBatch

    b = SgBatch()
    b.count, b.num_keys, b.flags = 4, 1, SG_BATCH_TLS
    b.keys, b.in_, b.out, b.status = 0x1000, 0x2000, 0x3000, 0x4000
    b.uniform_len, b.in_stride, b.out_stride = 64, 64, 80
    return b


def ext(ivs=0x5000, flags=0):
    from suruga_amd._native import SgBatchRfc8439

    x = SgBatchRfc8439()
    x.ivs, x.flags = ivs, flags
    return x


def test_extension_struct_layout():
    from suruga_amd._native import SgBatch, SgBatchRfc8439

    assert C.sizeof(SgBatchRfc8439) == 16
    assert (SgBatchRfc8439.ivs.offset, SgBatchRfc8439.flags.offset, SgBatchRfc8439._pad.offset) == (0, 8, 12)
    # the batch itself keeps its size and layout (include/suruga_gpu.h)
    assert C.sizeof(SgBatch) == 176
    assert (SgBatch.nonces.offset, SgBatch.in_.offset, SgBatch.workspace_size.offset) == (56, 80, 168)


@pytest.mark.parametrize("call", ["sg_seal_batch_rfc8439", "sg_open_batch_rfc8439"])
def test_rejections_before_any_gpu_call(lib, call):
    from suruga_amd._native import SG_BATCH_TLS, SG_E_ARG

    fn = getattr(lib, call)
    b = tls_batch()
    x = ext()
    assert fn(None, C.byref(x)) == SG_E_ARG and b"batch is NULL" in lib.sg_last_error()
    assert fn(C.byref(b), None) == SG_E_ARG and b"sg_batch_rfc8439 is NULL" in lib.sg_last_error()
    for flags in (1, 0x100, 0x80000000):
        assert fn(C.byref(b), C.byref(ext(flags=flags))) == SG_E_ARG
        assert b"flags must be 0" in lib.sg_last_error()
    for ivs in (0x5001, 0x5002, 0x5003):
        assert fn(C.byref(b), C.byref(ext(ivs=ivs))) == SG_E_ARG
        assert b"4-byte aligned" in lib.sg_last_error()
    assert fn(C.byref(b), C.byref(ext(ivs=None))) == SG_E_ARG and b"write IVs" in lib.sg_last_error()
    for bad in (0x4, 0x8, 0x100, 0x80000000):
        b.flags = SG_BATCH_TLS | bad
        assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"unknown flags" in lib.sg_last_error()
    b.flags = SG_BATCH_TLS
    # ... and what the draft calls reject
    b.uniform_len = 40000 + (16 if "open" in call else 0)
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"SG_MAX_RECORD_LEN" in lib.sg_last_error()
    b.uniform_len = 64
    b.keys = None
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"non-NULL" in lib.sg_last_error()
    b.count = 0
    assert fn(C.byref(b), C.byref(x)) == 0  # an empty batch is a no-op


def test_explicit_mode_rejections(lib):
    from suruga_amd._native import SG_E_ARG

    b = tls_batch()
    b.flags = 0
    x = ext(ivs=None)  # explicit mode takes no IVs
    assert lib.sg_seal_batch_rfc8439(C.byref(b), C.byref(x)) == SG_E_ARG and b"needs nonces" in lib.sg_last_error()
    b.nonces, b.ads, b.ad_len = 0x6000, 0x7000, 256
    assert lib.sg_seal_batch_rfc8439(C.byref(b), C.byref(x)) == SG_E_ARG and b"SG_MAX_AD_LEN" in lib.sg_last_error()
    b.ad_len, b.status = 13, None
    assert lib.sg_open_batch_rfc8439(C.byref(b), C.byref(x)) == SG_E_ARG and b"status" in lib.sg_last_error()


def test_draft_calls_still_reject_flag_4(lib):
    from suruga_amd._native import SG_BATCH_TLS, SG_E_ARG

    b = tls_batch()
    b.flags = SG_BATCH_TLS | 0x4
    for fn in (lib.sg_seal_batch, lib.sg_open_batch):
        assert fn(C.byref(b)) == SG_E_ARG and b"unknown flags" in lib.sg_last_error()


def test_python_batch_keeps_ivs_for_rfc8439():
    from suruga_amd import batch as B

    class T:  # a stand-in for a device tensor
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    bt = B.Batch(count=1, keys=T(0x1000), inp=T(0x2000), out=T(0x3000), rfc8439=True, ivs=T(0x5000))
    x = bt.to_c_rfc8439()
    assert (x.ivs, x.flags) == (0x5000, 0)
