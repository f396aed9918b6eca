"""One table of messages with exactly one defect each, through both entry points
of the message path: sg_seal_msg_dev / sg_open_msg_dev (one message) and
sg_seal_msg_batch / sg_open_msg_batch (the same message as an item of a
two-message batch).  Both must give the same code and the same
sg_last_error() text: the per-message checks are one function
(msg_check_args, suruga_amd/csrc/sg_msg_plan.h).

The cases and the made-up device addresses are those of
tests/test_msg_batch_abi.py.  Every case is decided on the host before any GPU
call and no pointer is dereferenced, so no GPU is needed.  The expected texts
are written down from the two call sites as they stood before the checks were
shared (run_msg in sg_msg_capi.cpp, run_msg_batch in sg_msg_batch_capi.cpp)."""
from __future__ import annotations

import ctypes as C

import pytest

from msg_batch_support import batch

NULLS = "in/out/ad must be non-NULL"
TOO_LONG = "message longer than SG_MSG_MAX_LEN"
AD_TOO_LONG = "ad_len exceeds SG_MSG_MAX_LEN"
OVERLAP = "out overlaps in (only out == in is allowed)"
MAX = 0xFFFFFFC0  # SG_MSG_MAX_LEN

# (name, open?, fields of the message to change, expected text); the well-formed
# message: ad 13 bytes, in 100 bytes, out elsewhere
CASES = [
    ("null-ad", False, {"ad": None}, NULLS),
    ("null-in", False, {"in_": None}, NULLS),
    ("null-out", False, {"out": None}, NULLS),
    ("null-ad-open", True, {"ad": None}, NULLS),
    ("null-in-open", True, {"in_": None}, NULLS),
    ("null-out-open", True, {"out": None}, NULLS),
    ("empty-seal-null-out", False, {"in_": None, "in_len": 0, "out": None}, NULLS),  # a tag is still written
    ("n-bound-seal", False, {"in_len": MAX + 1}, TOO_LONG),
    ("n-bound-open", True, {"in_len": MAX + 17}, TOO_LONG),  # open: n = in_len - 16
    ("ad-bound-seal", False, {"ad_len": MAX + 1}, AD_TOO_LONG),
    ("ad-bound-open", True, {"ad_len": MAX + 1}, AD_TOO_LONG),
    ("overlap-ahead", False, {"out": +1}, OVERLAP),            # out = in + 1
    ("overlap-tag-reaches-in", False, {"out": -100}, OVERLAP),  # out = in - 100: the tag reaches into in
    ("overlap-open", True, {"in_len": 116, "out": +115}, OVERLAP),
]


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def apply(obj, changes):
    for field, value in changes.items():
        if field == "out" and isinstance(value, int):
            value = obj.in_ + value  # relative to in
        setattr(obj, field, value)


def via_single(lib, open_, changes):
    from suruga_amd._native import SgMsg, load

    b, items = batch()
    it = items[1]
    m = SgMsg()
    m.key, m.status = 0x1000, 0x2000
    m.ad, m.ad_len, m.in_, m.in_len, m.out = it.ad, it.ad_len, it.in_, it.in_len, it.out
    m.flags, m.stream = 0, None
    m.workspace, m.workspace_size = 0x800000, load().sg_msg_workspace_size()
    apply(m, changes)
    rc = (lib.sg_open_msg_dev if open_ else lib.sg_seal_msg_dev)(C.byref(m))
    return rc, lib.sg_last_error()


def via_batch(lib, open_, changes):
    b, items = batch()
    apply(items[1], changes)
    rc = (lib.sg_open_msg_batch if open_ else lib.sg_seal_msg_batch)(C.byref(b))
    return rc, lib.sg_last_error()


@pytest.mark.parametrize("name,open_,changes,text", CASES, ids=[c[0] for c in CASES])
def test_one_defect_same_code_and_text_from_both_entry_points(lib, name, open_, changes, text):
    from suruga_amd._native import SG_E_ARG

    one = via_single(lib, open_, changes)
    many = via_batch(lib, open_, changes)
    assert one == (SG_E_ARG, text.encode()), one
    assert many == (SG_E_ARG, text.encode()), many
