"""CPU tests of the long-message plan (sg_msg_plan_for, suruga_amd/csrc/
sg_msg_plan.cpp) and of the argument errors of the message entry points that
need no device.  The plan checked here is the struct the kernels of sg_msg.hip
take as their argument."""
from __future__ import annotations

import ctypes as C

import pytest

ADLENS = [0, 1, 7, 8, 13, 255, 256, 4096, 70001]
GROUPS = [0, 1, 2, 3, 7]
U32 = 2**32
U64 = 2**64


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def check_plan(p: dict, n: int, adlen: int, groups: int) -> None:
    B = (adlen + 16 + n + 15) // 16
    assert p["mac_blocks"] == B
    K, T, z = p["tile_blocks"], p["tiles"], p["zero_blocks"]
    assert K >= 1 and p["tile_bytes"] == 16 * K
    assert z + B == T * K and 0 <= z < K
    G, per = p["groups"], p["tiles_per_group"]
    assert G >= 1 and per >= 1
    if groups:
        assert G <= groups
    # group g owns tiles [g * per, min(T, (g + 1) * per)): a partition of [0, T), no group empty
    assert (G - 1) * per < T <= G * per
    # nothing the kernels compute from the plan leaves 64 bits (or 63, signed byte offsets)
    assert T * K * 16 < 2**63 and G * per < U64
    assert all(p[f] < U32 for f in ("tile_blocks", "tile_bytes", "groups", "tiles_per_group"))
    assert T - per < 2**20 or T <= per  # the finish kernel's exponents (tiles after a group)


def test_plan_sweep():
    from suruga_amd import msg

    for n in range(0, 70001, 997):
        for adlen in ADLENS:
            for groups in GROUPS:
                check_plan(msg.plan_for(n, adlen, groups), n, adlen, groups)


def test_plan_small_ranges_partition_exactly():
    """The tile ranges spelled out: every tile in exactly one group."""
    from suruga_amd import msg

    for n in (0, 1, 16303, 16304, 16305, 50000, 70000):
        for groups in GROUPS:
            p = msg.plan_for(n, 13, groups)
            seen = []
            for g in range(p["groups"]):
                lo, hi = g * p["tiles_per_group"], min(p["tiles"], (g + 1) * p["tiles_per_group"])
                assert lo < hi
                seen += list(range(lo, hi))
            assert seen == list(range(p["tiles"]))


def test_plan_at_and_above_the_bound(lib):
    from suruga_amd import _native as N
    from suruga_amd import msg

    M = N.SG_MSG_MAX_LEN
    assert M == 0xFFFFFFC0
    for groups in GROUPS:
        check_plan(msg.plan_for(M, M, groups), M, M, groups)
        check_plan(msg.plan_for(M, 0, groups), M, 0, groups)
    p = N.SgMsgPlan()
    assert lib.sg_msg_plan_for(M + 1, 0, 0, C.byref(p)) == N.SG_E_ARG
    assert lib.sg_msg_plan_for(0, M + 1, 0, C.byref(p)) == N.SG_E_ARG
    assert lib.sg_msg_plan_for(2**64 - 1, 2**64 - 1, 0, C.byref(p)) == N.SG_E_ARG
    assert lib.sg_msg_plan_for(0, 0, 0, None) == N.SG_E_ARG
    with pytest.raises(N.NativeError):
        msg.plan_for(M + 1, 0)


def test_automatic_grid_is_bounded_by_the_workspace(lib):
    from suruga_amd import msg

    p = msg.plan_for(1 << 30, 13)
    assert p["groups"] * 32 <= lib.sg_msg_workspace_size()
    assert msg.plan_for(1 << 30, 13, 5000)["groups"] * 32 <= lib.sg_msg_workspace_size()


def test_set_msg_groups_switch(lib):
    prev = lib.sg_set_msg_groups(3)
    try:
        assert lib.sg_set_msg_groups(-1) == 3          # a negative argument only queries
        assert lib.sg_set_msg_groups(0) == 3           # returns the previous setting
        assert lib.sg_set_msg_groups(-1) == 0
    finally:
        lib.sg_set_msg_groups(prev)


def test_msg_device_form_argument_errors_without_gpu(lib):
    from suruga_amd._native import SG_E_ARG, SG_E_SHORT, SG_MSG_KEEP_FAILED, SG_MSG_MAX_LEN, SgMsg

    assert lib.sg_seal_msg_dev(None) == SG_E_ARG
    assert lib.sg_open_msg_dev(None) == SG_E_ARG

    def msg(**kw):
        m = SgMsg()
        m.key, m.ad, m.in_, m.out, m.status = 0x1000, 0x2000, 0x100000, 0x900000, 0x3000
        m.ad_len, m.in_len = 13, 4096
        for k, v in kw.items():
            setattr(m, k, v)
        return m

    assert lib.sg_seal_msg_dev(C.byref(msg(flags=0x2))) == SG_E_ARG and b"unknown flags" in lib.sg_last_error()
    assert lib.sg_open_msg_dev(C.byref(msg(flags=SG_MSG_KEEP_FAILED | 0x4))) == SG_E_ARG
    # open: fewer than 16 bytes is SG_E_SHORT before anything else is looked at
    assert lib.sg_open_msg_dev(C.byref(msg(in_len=15, key=None, out=None))) == SG_E_SHORT
    for field in ("key", "in_", "out", "ad"):
        assert lib.sg_seal_msg_dev(C.byref(msg(**{field: None}))) == SG_E_ARG
        assert b"non-NULL" in lib.sg_last_error()
    assert lib.sg_open_msg_dev(C.byref(msg(status=None))) == SG_E_ARG and b"status" in lib.sg_last_error()
    # lengths above the bound name the constant
    assert lib.sg_seal_msg_dev(C.byref(msg(in_len=SG_MSG_MAX_LEN + 1))) == SG_E_ARG
    assert b"SG_MSG_MAX_LEN" in lib.sg_last_error()
    assert lib.sg_open_msg_dev(C.byref(msg(in_len=SG_MSG_MAX_LEN + 17))) == SG_E_ARG
    assert b"SG_MSG_MAX_LEN" in lib.sg_last_error()
    assert lib.sg_seal_msg_dev(C.byref(msg(ad_len=SG_MSG_MAX_LEN + 1))) == SG_E_ARG
    assert b"SG_MSG_MAX_LEN" in lib.sg_last_error()
    # out may equal in exactly; any other overlap is refused (seal writes n + 16 bytes)
    for out in (0x100000 + 1, 0x100000 + 4095, 0x100000 - 1, 0x100000 - 4111):
        assert lib.sg_seal_msg_dev(C.byref(msg(out=out))) == SG_E_ARG and b"overlaps" in lib.sg_last_error()
    assert lib.sg_open_msg_dev(C.byref(msg(out=0x100000 + 16))) == SG_E_ARG and b"overlaps" in lib.sg_last_error()


def test_msg_host_form_argument_errors_without_gpu(lib):
    from suruga_amd._native import SG_E_ARG, SG_E_SHORT, SG_MSG_MAX_LEN

    out = (C.c_uint8 * 64)()
    dummy = C.cast(C.create_string_buffer(512), C.c_void_p)  # never dereferenced on these paths
    assert lib.sg_seal_msg(None, bytes(8), 8, b"", 0, b"", 0, out) == SG_E_ARG
    assert lib.sg_open_msg(None, bytes(8), 8, bytes(16), 16, b"", 0, out) == SG_E_ARG
    assert lib.sg_seal_msg(dummy, bytes(7), 7, b"", 0, b"", 0, out) == SG_E_ARG and b"nonce" in lib.sg_last_error()
    assert lib.sg_seal_msg(dummy, bytes(8), 8, None, 5, b"", 0, out) == SG_E_ARG
    assert lib.sg_seal_msg(dummy, bytes(8), 8, b"abc", 3, None, 4, out) == SG_E_ARG
    assert lib.sg_seal_msg(dummy, bytes(8), 8, b"abc", 3, b"", 0, None) == SG_E_ARG
    assert lib.sg_open_msg(dummy, bytes(8), 8, bytes(15), 15, b"", 0, out) == SG_E_SHORT
    assert lib.sg_seal_msg(dummy, bytes(8), 8, b"x", SG_MSG_MAX_LEN + 1, b"", 0, out) == SG_E_ARG
    assert b"SG_MSG_MAX_LEN" in lib.sg_last_error()
    assert lib.sg_seal_msg(dummy, bytes(8), 8, b"x", 1, b"x", SG_MSG_MAX_LEN + 1, out) == SG_E_ARG
    assert b"SG_MSG_MAX_LEN" in lib.sg_last_error()
