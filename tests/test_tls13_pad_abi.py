"""CPU tests of the padded TLS 1.3 seal's C boundary (sg_seal_batch_tls13_ex,
sg_tls13_seal_opts, sg_tls13_inner_len, include/suruga_gpu.h): the options struct's
layout, the header's prototypes, the inner length against RFC 8446 section 5.4's rule,
and every rejection -- all made before any GPU call (there is no GPU here)."""
from __future__ import annotations

import ctypes as C
from pathlib import Path

import pytest

from tls13_pad_support import inner_len  # RFC 8446 section 5.4, restated in Python once

N = 1 << 14
LENS = (0, 1, 62, 63, 64, 127, 4095, 4096, 16383, 16384)
PADS = (0, 1, 2, 64, 100, 256, 16384)


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def tls_batch(count=4):
    """A small uniform TLS 1.3 seal of made-up device addresses."""
    from suruga_amd._native import SG_BATCH_TLS, SgBatch

    b = SgBatch()
    b.count, b.num_keys, b.flags = count, 1, SG_BATCH_TLS
    b.keys, b.in_, b.out = 0x1000, 0x20000, 0x300000
    b.content_type = 23
    b.uniform_len, b.in_stride, b.out_stride = 64, 64, 160
    return b


def ext(ivs=0x5000, flags=0):
    from suruga_amd._native import SgBatchTls13

    x = SgBatchTls13()
    x.ivs, x.flags = ivs, flags
    return x


def opts(inner_types=None, pad_to=64, flags=0):
    from suruga_amd._native import SgTls13SealOpts

    o = SgTls13SealOpts()
    o.inner_types, o.pad_to, o.flags = inner_types, pad_to, flags
    return o


def err(lib) -> bytes:
    return lib.sg_last_error()


def test_options_struct_layout():
    from suruga_amd._native import SG_TLS13_MAX_INNER, SgBatchTls13, SgTls13SealOpts as O

    assert C.sizeof(O) == 16
    assert (O.inner_types.offset, O.pad_to.offset, O.flags.offset) == (0, 8, 12)
    assert SG_TLS13_MAX_INNER == N + 1
    assert C.sizeof(SgBatchTls13) == 32  # the extension struct of the plain calls is as it was


def test_header_declares_what_the_binding_mirrors():
    h = (Path(__file__).resolve().parent.parent / "include" / "suruga_gpu.h").read_text()
    for s in ("#define SG_TLS13_MAX_INNER (16384u + 1u)", "uint32_t sg_tls13_inner_len(uint32_t len, uint32_t pad_to);",
              "typedef struct sg_tls13_seal_opts {", "    const uint8_t* inner_types;", "    uint32_t       pad_to;",
              "    uint32_t       flags;", "} sg_tls13_seal_opts;",
              "int sg_seal_batch_tls13_ex(const sg_batch* b, const sg_batch_tls13* x, const sg_tls13_seal_opts* o);",
              # ... beside the calls it extends, which keep their prototypes
              "int sg_seal_batch_tls13(const sg_batch* b, const sg_batch_tls13* x);",
              "int sg_open_batch_tls13(const sg_batch* b, const sg_batch_tls13* x);",
              "int sg_batch_tls13_route(const sg_batch* b, int open);"):
        assert s in h, s


@pytest.mark.parametrize("pad_to", PADS)
def test_inner_len(lib, pad_to):
    from suruga_amd import batch as B

    for n in LENS:
        assert lib.sg_tls13_inner_len(n, pad_to) == inner_len(n, pad_to), (n, pad_to)
        assert B.tls13_inner_len(n, pad_to) == inner_len(n, pad_to), (n, pad_to)


def test_inner_len_of_the_rfc_examples(lib):
    """The static_asserts of sg_layout.h, through the exported function."""
    for n, pad_to, want in ((0, 64, 64), (63, 64, 64), (64, 64, 128), (16384, 64, 16385), (100, 100, 200)):
        assert lib.sg_tls13_inner_len(n, pad_to) == want


def test_rejections_before_any_gpu_call(lib):
    from suruga_amd._native import SG_BATCH_KEEP_FAILED, SG_BATCH_TLS, SG_E_ARG

    fn = lib.sg_seal_batch_tls13_ex
    b, x, o = tls_batch(), ext(), opts()
    # the options
    assert fn(C.byref(b), C.byref(x), None) == SG_E_ARG and b"sg_tls13_seal_opts is NULL" in err(lib)
    for flags in (1, 0x100, 0x80000000):
        assert fn(C.byref(b), C.byref(x), C.byref(opts(flags=flags))) == SG_E_ARG
        assert b"sg_tls13_seal_opts.flags must be 0" in err(lib)
    for pad_to in (N + 1, 1 << 15, 0xFFFFFFFF):
        assert fn(C.byref(b), C.byref(x), C.byref(opts(pad_to=pad_to))) == SG_E_ARG and b"pad_to above 2^14" in err(lib)
    # everything sg_seal_batch_tls13 rejects, with its texts
    assert fn(None, C.byref(x), C.byref(o)) == SG_E_ARG and b"batch is NULL" in err(lib)
    assert fn(C.byref(b), None, C.byref(o)) == SG_E_ARG and b"sg_batch_tls13 is NULL" in err(lib)
    for flags in (1, 0x100, 0x80000000):
        assert fn(C.byref(b), C.byref(ext(flags=flags)), C.byref(o)) == SG_E_ARG
        assert b"sg_batch_tls13.flags must be 0" in err(lib)
    for flags in (0, SG_BATCH_KEEP_FAILED):
        b.flags = flags
        assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"SG_BATCH_TLS must be set" in err(lib)
    for bad in (0x4, 0x8, 0x100, 0x80000000):
        b.flags = SG_BATCH_TLS | bad
        assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"unknown flags" in err(lib)
    b.flags = SG_BATCH_TLS
    assert fn(C.byref(b), C.byref(ext(ivs=None)), C.byref(o)) == SG_E_ARG and b"write IVs" in err(lib)
    for ivs in (0x5001, 0x5002, 0x5003):
        assert fn(C.byref(b), C.byref(ext(ivs=ivs)), C.byref(o)) == SG_E_ARG and b"4-byte aligned" in err(lib)
    # max_len / uniform_len bound the content, whatever the padding makes of it
    b.uniform_len = N + 1
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"2^14 bytes" in err(lib)
    b.uniform_len, b.len, b.max_len = 0, 0x8000, N + 1
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"2^14 bytes" in err(lib)
    b.len, b.max_len, b.uniform_len = None, 0, 64
    b.content_type = 0
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"must be non-zero" in err(lib)
    b.content_type = 23
    b.keys = None
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"non-NULL" in err(lib)
    b.keys = 0x1001
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"key table must be 4-byte aligned" in err(lib)
    b.keys, b.num_keys = 0x1000, 0
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"num_keys" in err(lib)
    b.num_keys, b.len = 1, 0x8000  # a length array without max_len
    assert fn(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG and b"max_len is required" in err(lib)
    b.len, b.count = None, 0
    for o in (opts(), opts(pad_to=0), opts(pad_to=1), opts(pad_to=N), opts(pad_to=100)):
        assert fn(C.byref(b), C.byref(x), C.byref(o)) == 0  # an empty batch is a no-op


def test_zero_content_type_with_per_record_types(lib):
    """b->content_type is not read when the records bring their own types: a zero there is
    accepted, and the call goes on to its other checks."""
    from suruga_amd._native import SG_E_ARG

    fn = lib.sg_seal_batch_tls13_ex
    b, x = tls_batch(), ext()
    b.content_type = 0
    typed = opts(inner_types=0x8000)
    assert fn(C.byref(b), C.byref(x), C.byref(opts())) == SG_E_ARG and b"must be non-zero" in err(lib)
    b.keys = None  # the next check in line
    assert fn(C.byref(b), C.byref(x), C.byref(typed)) == SG_E_ARG and b"non-NULL" in err(lib)
    b.keys, b.uniform_len = 0x1000, N + 1
    assert fn(C.byref(b), C.byref(x), C.byref(typed)) == SG_E_ARG and b"2^14 bytes" in err(lib)
    b.uniform_len, b.count = N, 0
    assert fn(C.byref(b), C.byref(x), C.byref(typed)) == 0
    # the plain call still rejects the zero
    assert lib.sg_seal_batch_tls13(C.byref(b), C.byref(x)) == SG_E_ARG and b"must be non-zero" in err(lib)


def test_python_wrappers():
    import inspect

    from suruga_amd import _native as Nt
    from suruga_amd import batch as B

    assert {"sg_seal_batch_tls13_ex", "sg_tls13_inner_len"} <= set(Nt.EXPORTS)
    sig = inspect.signature(B.seal_tls13)
    assert list(sig.parameters) == ["batch", "pad_to", "inner_types"]
    assert sig.parameters["pad_to"].default == 0 and sig.parameters["inner_types"].default is None
    assert callable(B.tls13_inner_len)
