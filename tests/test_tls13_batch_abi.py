"""CPU tests of the TLS 1.3 record batch's C boundary (sg_seal_batch_tls13 /
sg_open_batch_tls13 / sg_batch_tls13_route, include/suruga_gpu.h): the extension
struct's layout, every rejection -- all made before any GPU call (there is no GPU
here) -- and the route predicate over the eligible shape and each way to miss it."""
from __future__ import annotations

import ctypes as C

import pytest

N = 1 << 14


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def tls_batch(open_=False):
    """A small uniform TLS 1.3 batch of made-up device addresses."""
    from suruga_amd._native import SG_BATCH_TLS, SgBatch

    b = SgBatch()
    b.count, b.num_keys, b.flags = 4, 1, SG_BATCH_TLS
    b.keys, b.in_, b.out, b.status = 0x1000, 0x20000, 0x300000, 0x4000
    b.content_type = 23
    b.uniform_len, b.in_stride, b.out_stride = (81, 96, 64) if open_ else (64, 64, 96)
    return b


def full_batch(open_):
    """The shape the wave-per-record kernel takes: full records, 16-byte aligned."""
    b = tls_batch(open_)
    b.uniform_len = N + 17 if open_ else N
    b.in_stride, b.out_stride = (N + 32, N + 16) if open_ else (N, N + 32)
    return b


def ext(ivs=0x5000, inner_type=0x6000, content_len=0x7000, flags=0):
    from suruga_amd._native import SgBatchTls13

    x = SgBatchTls13()
    x.ivs, x.inner_type, x.content_len, x.flags = ivs, inner_type, content_len, flags
    return x


def err(lib) -> bytes:
    return lib.sg_last_error()


def test_extension_struct_layout():
    from suruga_amd._native import SG_STATUS_NO_TYPE, SgBatch, SgBatchRfc8439, SgBatchTls13 as X

    assert C.sizeof(X) == 32
    assert (X.ivs.offset, X.inner_type.offset, X.content_len.offset, X.flags.offset, X._pad.offset) == (0, 8, 16, 24, 28)
    assert SG_STATUS_NO_TYPE == 5
    # the batch and the RFC extension keep their size and layout
    assert C.sizeof(SgBatch) == 176 and C.sizeof(SgBatchRfc8439) == 16


def test_header_declares_what_the_binding_mirrors():
    from pathlib import Path

    h = (Path(__file__).resolve().parent.parent / "include" / "suruga_gpu.h").read_text()
    for s in ("typedef struct sg_batch_tls13 {", "int sg_seal_batch_tls13(const sg_batch* b, const sg_batch_tls13* x);",
              "int sg_open_batch_tls13(const sg_batch* b, const sg_batch_tls13* x);", "#define SG_STATUS_NO_TYPE 5",
              "int sg_batch_tls13_route(const sg_batch* b, int open);"):
        assert s in h, s


@pytest.mark.parametrize("call", ["sg_seal_batch_tls13", "sg_open_batch_tls13"])
def test_rejections_before_any_gpu_call(lib, call):
    from suruga_amd._native import SG_BATCH_KEEP_FAILED, SG_BATCH_TLS, SG_E_ARG

    fn = getattr(lib, call)
    open_ = "open" in call
    b, x = tls_batch(open_), ext()
    assert fn(None, C.byref(x)) == SG_E_ARG and b"batch is NULL" in err(lib)
    assert fn(C.byref(b), None) == SG_E_ARG and b"sg_batch_tls13 is NULL" in err(lib)
    for flags in (1, 0x100, 0x80000000):
        assert fn(C.byref(b), C.byref(ext(flags=flags))) == SG_E_ARG and b"sg_batch_tls13.flags must be 0" in err(lib)
    # the batch's flags: TLS mode is required, KEEP_FAILED allowed, nothing else
    for flags in (0, SG_BATCH_KEEP_FAILED):
        b.flags = flags
        assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"SG_BATCH_TLS must be set" in err(lib)
    for bad in (0x4, 0x8, 0x100, 0x80000000):
        b.flags = SG_BATCH_TLS | bad
        assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"unknown flags" in err(lib)
    b.flags = SG_BATCH_TLS
    # the IVs
    assert fn(C.byref(b), C.byref(ext(ivs=None))) == SG_E_ARG and b"write IVs" in err(lib)
    for ivs in (0x5001, 0x5002, 0x5003):
        assert fn(C.byref(b), C.byref(ext(ivs=ivs))) == SG_E_ARG and b"4-byte aligned" in err(lib)
    # the length bounds (RFC 8446 section 5.1 / 5.2), uniform and listed
    over = N + 256 + 1 if open_ else N + 1
    what = b"2^14 + 256" if open_ else b"2^14 bytes"
    b.uniform_len = over
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and what in err(lib)
    b.uniform_len, b.len, b.max_len = 0, 0x8000, over
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and what in err(lib)
    b.len, b.max_len, b.uniform_len = None, 0, tls_batch(open_).uniform_len
    if open_:
        assert fn(C.byref(b), C.byref(ext(inner_type=None))) == SG_E_ARG and b"inner_type and content_len" in err(lib)
        assert fn(C.byref(b), C.byref(ext(content_len=None))) == SG_E_ARG and b"inner_type and content_len" in err(lib)
        for cl in (0x7001, 0x7002, 0x7003):
            assert fn(C.byref(b), C.byref(ext(content_len=cl))) == SG_E_ARG and b"content_len must be 4-byte" in err(lib)
        b.status = None
        assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"status" in err(lib)
        b.status = 0x4000
    else:
        b.content_type = 0
        assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"must be non-zero" in err(lib)
        b.content_type = 23
        # seal reads neither output array
        assert fn(C.byref(tls_batch_empty()), C.byref(ext(inner_type=None, content_len=None))) == 0
    # ... and what the RFC calls reject
    b.keys = None
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"non-NULL" in err(lib)
    b.keys = 0x1001
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"key table must be 4-byte aligned" in err(lib)
    b.keys, b.num_keys = 0x1000, 0
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"num_keys" in err(lib)
    b.num_keys, b.len = 1, 0x8000  # a length array without max_len
    assert fn(C.byref(b), C.byref(x)) == SG_E_ARG and b"max_len is required" in err(lib)
    b.len, b.count = None, 0
    assert fn(C.byref(b), C.byref(x)) == 0  # an empty batch is a no-op


def tls_batch_empty():
    b = tls_batch()
    b.count = 0
    return b


def test_the_largest_lengths_pass_the_checks(lib):
    """2^14 content bytes and a 2^14 + 256 byte fragment are inside the bounds: with
    count 0 the call reaches its end without a GPU."""
    for fn, n in ((lib.sg_seal_batch_tls13, N), (lib.sg_open_batch_tls13, N + 256)):
        b = tls_batch_empty()
        b.uniform_len = n
        assert fn(C.byref(b), C.byref(ext())) == 0


def test_rfc_and_draft_calls_are_as_they_were(lib):
    from suruga_amd._native import SG_BATCH_TLS, SG_E_ARG, SgBatchRfc8439

    b = tls_batch()
    x = SgBatchRfc8439()
    x.ivs, x.flags = 0x5000, 1
    assert lib.sg_seal_batch_rfc8439(C.byref(b), C.byref(x)) == SG_E_ARG and b"sg_batch_rfc8439.flags must be 0" in err(lib)
    b.flags = SG_BATCH_TLS | 0x4
    for fn in (lib.sg_seal_batch, lib.sg_open_batch):
        assert fn(C.byref(b)) == SG_E_ARG and b"unknown flags" in err(lib)


@pytest.mark.parametrize("open_", [False, True])
def test_route(lib, open_):
    from suruga_amd._native import SG_BATCH_TLS, SG_E_ARG

    route = lib.sg_batch_tls13_route
    o = 1 if open_ else 0
    assert lib.sg_set_lockstep(-1) == 1  # the default
    assert route(C.byref(full_batch(open_)), o) == 1
    # the same batch read the other way round: a seal's 2^14 is no full fragment, and
    # an open's 2^14 + 17 is more content than a record holds
    assert route(C.byref(full_batch(open_)), 1 - o) == (SG_E_ARG if open_ else 0)

    def miss(**kw):
        b = full_batch(open_)
        for k, v in kw.items():
            setattr(b, k, v)
        return route(C.byref(b), o)

    full = N + 17 if open_ else N
    for n in (full - 1, full + 1 if open_ else full - 64, 64 + 17):  # length
        assert miss(uniform_len=n) == 0
    assert miss(in_stride=full_batch(open_).in_stride + 8) == 0   # strides
    assert miss(out_stride=full_batch(open_).out_stride + 4) == 0
    assert miss(in_=0x20008) == 0 and miss(out=0x300001) == 0     # bases
    assert miss(key_index=0x9002) == 0 and miss(seq=0xA004 + 2) == 0
    assert miss(key_index=0x9004, seq=0xA008) == 1
    assert miss(len=0x8000, max_len=full, uniform_len=0) == 0     # len / offsets given
    assert miss(in_off=0xB000) == 0 and miss(out_off=0xC000) == 0
    prev = lib.sg_set_lockstep(0)                                  # lockstep off
    try:
        assert route(C.byref(full_batch(open_)), o) == 0
    finally:
        lib.sg_set_lockstep(prev)
    assert route(C.byref(full_batch(open_)), o) == 1
    # what the calls reject of the batch itself
    assert route(None, o) == SG_E_ARG and b"batch is NULL" in err(lib)
    assert miss(flags=0) == SG_E_ARG and miss(flags=SG_BATCH_TLS | 4) == SG_E_ARG
    assert miss(uniform_len=N + 256 + 1 if open_ else N + 1) == SG_E_ARG
    if not open_:
        assert miss(content_type=0) == SG_E_ARG


def test_python_batch_carries_the_tls13_fields():
    from suruga_amd import batch as B

    class T:  # a stand-in for a device tensor
        def __init__(self, p):
            self.p = p

        def data_ptr(self):
            return self.p

    bt = B.Batch(count=1, keys=T(0x1000), inp=T(0x2000), out=T(0x3000), ivs=T(0x5000), inner_type=T(0x6000),
                 content_len=T(0x7000))
    x = bt.to_c_tls13()
    assert (x.ivs, x.inner_type, x.content_len, x.flags) == (0x5000, 0x6000, 0x7000, 0)
    assert {"seal_tls13", "open_tls13", "tls13_route"} <= set(dir(B))
