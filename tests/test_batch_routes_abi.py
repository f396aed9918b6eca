"""CPU tests of sg_last_batch_routes (include/suruga_gpu.h): the struct's layout, the
NULL rejection, and what the diagnostic says before any batch has classified its
records (there is no GPU here)."""
from __future__ import annotations

import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def test_struct_layout():
    from suruga_amd._native import SgBatchRoutes as T

    assert C.sizeof(T) == 32
    assert (T.known.offset, T.classes.offset, T.bucket.offset, T.packed.offset, T.skipped.offset, T._pad.offset) == \
        (0, 4, 8, 20, 24, 28)
    assert T.bucket.size == 12


def test_null_is_rejected(lib):
    from suruga_amd._native import SG_E_ARG

    assert lib.sg_last_batch_routes(None) == SG_E_ARG
    assert b"sg_batch_routes is NULL" in lib.sg_last_error()


def test_unknown_without_a_classified_batch(lib):
    """A rejected call and an empty one classify nothing: known stays 0."""
    from suruga_amd import batch as B
    from suruga_amd._native import SG_E_ARG, SgBatch, SgBatchRoutes

    r = SgBatchRoutes()
    for i in range(8):
        C.cast(C.byref(r), C.POINTER(C.c_uint32))[i] = 0xDEADBEEF
    assert lib.sg_seal_batch(None) == SG_E_ARG
    assert lib.sg_last_batch_routes(C.byref(r)) == 0
    assert (r.known, r.classes, list(r.bucket), r.packed, r.skipped, r._pad) == (0, 0, [0, 0, 0], 0, 0, 0)
    b = SgBatch()  # count 0: a no-op
    assert lib.sg_open_batch(C.byref(b)) == 0
    assert B.last_routes() == {"known": False, "classes": 0, "bucket": [0, 0, 0], "packed": 0, "skipped": 0}
