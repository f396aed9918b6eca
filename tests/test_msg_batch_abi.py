"""The message batch's argument checks (sg_seal_msg_batch / sg_open_msg_batch):
every SG_E_ARG case of include/suruga_gpu.h is decided on the host before any
GPU call, so all of them are pinned here without a GPU (the pointers are never
dereferenced on these paths), and sg_msg_batch_workspace_size grows with count."""
from __future__ import annotations

import ctypes as C

import pytest

from msg_batch_support import batch, rejected


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def test_null_batch_and_empty_batch(lib):
    from suruga_amd._native import SG_E_ARG, SG_OK, SgMsgBatch

    assert lib.sg_seal_msg_batch(None) == SG_E_ARG
    assert lib.sg_open_msg_batch(None) == SG_E_ARG
    b = SgMsgBatch()  # count 0, everything NULL: nothing to do, nothing launched
    assert lib.sg_seal_msg_batch(C.byref(b)) == SG_OK
    assert lib.sg_open_msg_batch(C.byref(b)) == SG_OK


def test_flags_count_and_tables(lib):
    from suruga_amd._native import SG_MSG_BATCH_MAX_COUNT, SG_MSG_KEEP_FAILED

    b, _ = batch()
    b.flags = SG_MSG_KEEP_FAILED | 0x2
    rejected(lib, b, text="unknown flags")
    rejected(lib, b, open_=True, text="unknown flags")
    b, _ = batch()
    b.count = SG_MSG_BATCH_MAX_COUNT + 1
    rejected(lib, b, text="SG_MSG_BATCH_MAX_COUNT")
    for field in ("keys", "items"):
        b, _ = batch()
        setattr(b, field, None)
        rejected(lib, b, text="non-NULL")
    b, _ = batch()
    b.num_keys = 0
    rejected(lib, b)
    b, _ = batch()
    b.status = None
    rejected(lib, b, open_=True, text="status")


def test_workspace(lib):
    b, _ = batch()
    b.workspace_size -= 1
    rejected(lib, b, text="too small")
    b, _ = batch()
    b.workspace += 8
    rejected(lib, b, text="16-byte aligned")


def test_items(lib):
    from suruga_amd._native import SG_MSG_MAX_LEN

    b, items = batch()
    items[1].key_index = 2  # num_keys is 2
    rejected(lib, b, text="key_index")
    rejected(lib, b, open_=True, text="key_index")
    for field in ("ad", "in_", "out"):
        b, items = batch()
        setattr(items[1], field, None)
        rejected(lib, b, text="non-NULL")
    b, items = batch()  # seal of an empty message still writes a tag
    items[0].in_, items[0].in_len, items[0].out = None, 0, None
    rejected(lib, b, text="non-NULL")
    b, items = batch()
    items[0].in_len = SG_MSG_MAX_LEN + 1
    rejected(lib, b, text="SG_MSG_MAX_LEN")
    b, items = batch()
    items[0].in_len = SG_MSG_MAX_LEN + 17  # open: n = in_len - 16
    rejected(lib, b, open_=True, text="SG_MSG_MAX_LEN")
    b, items = batch()
    items[1].ad_len = SG_MSG_MAX_LEN + 1
    rejected(lib, b, text="SG_MSG_MAX_LEN")


def test_overlap_within_a_message(lib):
    b, items = batch()
    items[1].out = items[1].in_ + 1
    rejected(lib, b, text="overlaps")
    b, items = batch()
    items[1].out = items[1].in_ - 100  # the tag reaches into in
    rejected(lib, b, text="overlaps")
    b, items = batch()
    items[1].in_len = 116
    items[1].out = items[1].in_ + 115
    rejected(lib, b, open_=True, text="overlaps")


def test_workspace_size_is_monotone_in_count(lib):
    from suruga_amd._native import SG_MSG_BATCH_MAX_COUNT

    counts = [0, 1, 2, 3, 13, 255, 256, 257, 3000, 1 << 16, SG_MSG_BATCH_MAX_COUNT]
    sizes = [lib.sg_msg_batch_workspace_size(c) for c in counts]
    assert all(a < b for a, b in zip(sizes, sizes[1:])), sizes
    assert all(s % 16 == 0 for s in sizes)
    # room for the tables of count messages and one partial per possible segment
    assert all(s >= c * (64 + 32 + 8 + 16 + 32) for c, s in zip(counts, sizes))
    assert lib.sg_msg_batch_workspace_size(SG_MSG_BATCH_MAX_COUNT + 1) == sizes[-1]
