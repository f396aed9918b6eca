"""CPU tests of the RFC 8439 side of the message path: the plans
(sg_msg_plan_for_flags, sg_msg_batch_plan_for_flags), the decomposition over the
planned tiles in Python integers, the argument errors that need no device and
the layout of the structs that gained nonce_hi in their padding."""
from __future__ import annotations

import ctypes as C

import pytest

import msg_batch_support as mbs
import rfc8439_ref as ref

ADLENS = [0, 1, 7, 8, 13, 15, 16, 17, 255, 256, 4096, 70001]
GROUPS = [0, 1, 2, 3, 7]
PLAN_FIELDS = ("mac_blocks", "tiles", "zero_blocks", "tile_blocks", "tile_bytes", "groups", "tiles_per_group")


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def plan_flags(lib, n, adlen, flags, groups):
    from suruga_amd import _native as N

    p = N.SgMsgPlan()
    rc = lib.sg_msg_plan_for_flags(n, adlen, flags, groups, C.byref(p))
    return rc, {f: int(getattr(p, f)) for f in PLAN_FIELDS}


def test_flags_zero_is_the_draft_plan_field_for_field(lib):
    from suruga_amd import msg
    from suruga_amd._native import SG_MSG_KEEP_FAILED, SG_OK

    for n in list(range(0, 70001, 1997)) + [0xFFFFFFC0]:
        for adlen in ADLENS:
            for groups in GROUPS:
                want = msg.plan_for(n, adlen, groups)
                assert plan_flags(lib, n, adlen, 0, groups) == (SG_OK, want)
                assert plan_flags(lib, n, adlen, SG_MSG_KEEP_FAILED, groups) == (SG_OK, want)


def check_rfc_plan(p: dict, n: int, adlen: int, groups: int) -> None:
    L = ref.stream_len(n, adlen)
    assert L % 16 == 0 and p["mac_blocks"] == L // 16
    K, T, z = p["tile_blocks"], p["tiles"], p["zero_blocks"]
    assert p["tile_bytes"] == 16 * K == ref.TB
    assert z + p["mac_blocks"] == T * K and 0 <= z < K
    G, per = p["groups"], p["tiles_per_group"]
    assert G >= 1 and per >= 1 and (not groups or G <= groups)
    assert (G - 1) * per < T <= G * per  # a partition of [0, T), no group empty


def test_rfc_plan_sweep(lib):
    from suruga_amd import msg
    from suruga_amd._native import SG_MSG_KEEP_FAILED, SG_MSG_RFC8439, SG_OK

    shapes = [(n, a) for n in range(0, 70001, 997) for a in ADLENS] + ref.single_shapes()
    shapes += [(0xFFFFFFC0, 0xFFFFFFC0), (0xFFFFFFC0, 0)]
    for n, adlen in shapes:
        for groups in GROUPS:
            p = msg.plan_for(n, adlen, groups, rfc8439=True)
            check_rfc_plan(p, n, adlen, groups)
            assert plan_flags(lib, n, adlen, SG_MSG_RFC8439 | SG_MSG_KEEP_FAILED, groups) == (SG_OK, p)


def test_rfc_stream_is_at_most_30_bytes_longer():
    from suruga_amd import msg

    for n, adlen in ref.single_shapes():
        d = 16 * (msg.plan_for(n, adlen, 0, rfc8439=True)["mac_blocks"] - msg.plan_for(n, adlen, 0)["mac_blocks"])
        assert -16 < ref.stream_len(n, adlen) - (adlen + 16 + n) <= 30 and abs(d) <= 32


def test_plan_errors(lib):
    from suruga_amd import _native as N
    from suruga_amd import msg

    M = N.SG_MSG_MAX_LEN
    for flags in (0x2, 0x4, 0x200, N.SG_MSG_RFC8439 | 0x2):
        assert plan_flags(lib, 100, 13, flags, 0)[0] == N.SG_E_ARG, hex(flags)
    assert plan_flags(lib, M + 1, 0, N.SG_MSG_RFC8439, 0)[0] == N.SG_E_ARG
    assert plan_flags(lib, 0, M + 1, N.SG_MSG_RFC8439, 0)[0] == N.SG_E_ARG
    assert lib.sg_msg_plan_for_flags(0, 0, N.SG_MSG_RFC8439, 0, None) == N.SG_E_ARG
    with pytest.raises(N.NativeError):
        msg.plan_for(M + 1, 0, rfc8439=True)
    n = (C.c_uint64 * 1)(100)
    a = (C.c_uint64 * 1)(13)
    plan = N.SgMsgBatchPlan()
    for flags, want in ((0, N.SG_OK), (N.SG_MSG_RFC8439, N.SG_OK), (0x2, N.SG_E_ARG), (0x4, N.SG_E_ARG),
                        (0x200, N.SG_E_ARG)):
        rc = lib.sg_msg_batch_plan_for_flags(n, a, 1, flags, 0, C.byref(plan), None, None, 0, None, None)
        assert rc == want, hex(flags)


@pytest.mark.parametrize("groups", mbs.GROUPS)
def test_batch_plan(groups):
    from suruga_amd import msg

    shapes = ref.batch_shapes()
    lens, adlens = [n for _, n in shapes], [a for a, _ in shapes]
    assert msg.batch_plan_for(lens, adlens, groups, rfc8439=False) == msg.batch_plan_for(lens, adlens, groups)
    plan = msg.batch_plan_for(lens, adlens, groups, rfc8439=True)
    mbs.check_plan(plan, shapes, groups, lambda n, adlen, g: msg.plan_for(n, adlen, g, rfc8439=True))
    for (adlen, n), pm in zip(shapes, plan["msgs"]):
        check_rfc_plan(pm, n, adlen, groups)
    assert plan["tile_bytes"] == ref.TB


@pytest.mark.parametrize("groups", [1, 2, 0])
def test_decomposition_over_the_planned_tiles_single(groups):
    """Tile by tile from the exported plan, the padded stream gives the sequential tag."""
    from suruga_amd import msg

    multi = 0
    for n, adlen in ref.single_shapes():
        key, nonce, _, ad = ref.single_message(n, adlen)
        sealed = ref.sealed_single(n, adlen)
        plan = ref.single_as_batch(msg.plan_for(n, adlen, groups, rfc8439=True))
        assert ref.decomposed_tags([(key, nonce, ad, sealed[:n])], plan) == [sealed[n:]], (n, adlen)
        if len(plan["segs"]) > 1:
            multi += 1
            assert ref.decomposed_tags([(key, nonce, ad, sealed[:n])], plan, exp_shift=1) != [sealed[n:]]
    assert (multi > 0) == (groups != 1)


@pytest.mark.parametrize("groups", [1, 3, 0])
def test_decomposition_over_the_planned_tiles_batch(groups):
    from suruga_amd import msg

    shapes, msgs = ref.batch_shapes(), ref.batch_messages()
    plan = msg.batch_plan_for([n for _, n in shapes], [a for a, _ in shapes], groups, rfc8439=True)
    tags = ref.decomposed_tags([(m.key, m.nonce, m.ad, m.sealed[:len(m.pt)]) for m in msgs], plan)
    assert tags == [m.sealed[len(m.pt):] for m in msgs]
    # the draft's plan cuts another stream: it does not fit these
    with pytest.raises(AssertionError):
        ref.decomposed_tags([(m.key, m.nonce, m.ad, m.sealed[:len(m.pt)]) for m in msgs],
                            msg.batch_plan_for([n for _, n in shapes], [a for a, _ in shapes], groups))


def test_struct_layout_is_unchanged():
    """nonce_hi lies in former padding: the sizes and offsets of SG_ABI_VERSION 1."""
    from suruga_amd._native import SgMsg, SgMsgBatch, SgMsgItem

    assert C.sizeof(SgMsg) == 96
    assert [(f, getattr(SgMsg, f).offset) for f in ("key", "nonce", "ad", "ad_len", "in_", "in_len", "out", "status",
                                                    "flags", "nonce_hi", "stream", "workspace", "workspace_size")] == \
        [("key", 0), ("nonce", 8), ("ad", 16), ("ad_len", 24), ("in_", 32), ("in_len", 40), ("out", 48), ("status", 56),
         ("flags", 64), ("nonce_hi", 68), ("stream", 72), ("workspace", 80), ("workspace_size", 88)]
    assert C.sizeof(SgMsgItem) == 56
    assert [(f, getattr(SgMsgItem, f).offset) for f in ("key_index", "nonce", "nonce_hi", "ad", "ad_len", "in_",
                                                        "in_len", "out")] == \
        [("key_index", 0), ("nonce", 4), ("nonce_hi", 12), ("ad", 16), ("ad_len", 24), ("in_", 32), ("in_len", 40),
         ("out", 48)]
    assert C.sizeof(SgMsgBatch) == 64 and SgMsgBatch.stream.offset == 40 and SgMsgBatch.items.offset == 24


def test_device_form_flags_without_gpu(lib):
    from suruga_amd._native import SG_E_ARG, SG_E_SHORT, SG_MSG_KEEP_FAILED, SG_MSG_RFC8439, SgMsg

    def m(**kw):
        s = SgMsg()
        s.key, s.ad, s.in_, s.out, s.status = 0x1000, 0x2000, 0x100000, 0x900000, 0x3000
        s.ad_len, s.in_len = 13, 4096
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    for flags in (0x2, 0x4, 0x200, SG_MSG_RFC8439 | 0x2, SG_MSG_RFC8439 | SG_MSG_KEEP_FAILED | 0x200):
        assert lib.sg_seal_msg_dev(C.byref(m(flags=flags))) == SG_E_ARG and b"unknown flags" in lib.sg_last_error()
        assert lib.sg_open_msg_dev(C.byref(m(flags=flags))) == SG_E_ARG and b"unknown flags" in lib.sg_last_error()
    # the flag is accepted: the call gets as far as the next check
    for flags in (SG_MSG_RFC8439, SG_MSG_RFC8439 | SG_MSG_KEEP_FAILED):
        assert lib.sg_seal_msg_dev(C.byref(m(flags=flags, key=None))) == SG_E_ARG
        assert b"key must be non-NULL" in lib.sg_last_error()
        assert lib.sg_open_msg_dev(C.byref(m(flags=flags, in_len=15))) == SG_E_SHORT
        assert lib.sg_seal_msg_dev(C.byref(m(flags=flags, out=0x100000 + 1))) == SG_E_ARG
        assert b"overlaps" in lib.sg_last_error()


def test_batch_flags_without_gpu(lib):
    from msg_batch_support import batch, rejected

    from suruga_amd._native import SG_MSG_KEEP_FAILED, SG_MSG_RFC8439

    for flags in (0x2, 0x4, 0x200, SG_MSG_RFC8439 | 0x4):
        b, _ = batch()
        b.flags = flags
        rejected(lib, b, text="unknown flags")
        rejected(lib, b, open_=True, text="unknown flags")
    for flags in (SG_MSG_RFC8439, SG_MSG_RFC8439 | SG_MSG_KEEP_FAILED):
        b, items = batch()
        b.flags = flags
        items[1].key_index = 2  # the flag passes; the next check speaks
        rejected(lib, b, text="key_index")
        rejected(lib, b, open_=True, text="key_index")


def test_host_forms_nonce_length_without_gpu(lib):
    from suruga_amd._native import SG_E_ARG, SG_E_SHORT

    out = (C.c_uint8 * 64)()
    dummy = C.cast(C.create_string_buffer(512), C.c_void_p)  # never dereferenced on these paths
    assert lib.sg_seal_msg_rfc8439(None, bytes(12), 12, b"", 0, b"", 0, out) == SG_E_ARG
    for f in (lib.sg_seal_msg_rfc8439, lib.sg_open_msg_rfc8439):
        for bad in (0, 8, 11, 13, 16):
            assert f(dummy, bytes(16), bad, bytes(16), 16, b"", 0, out) == SG_E_ARG
            assert b"nonce must be 12 bytes" in lib.sg_last_error()
        assert f(dummy, None, 12, bytes(16), 16, b"", 0, out) == SG_E_ARG
    for f in (lib.sg_seal_msg, lib.sg_open_msg):  # the draft forms keep refusing anything but 8
        assert f(dummy, bytes(12), 12, bytes(16), 16, b"", 0, out) == SG_E_ARG
        assert b"nonce must be 8 bytes" in lib.sg_last_error()
    # 12 bytes pass: the next checks speak
    assert lib.sg_seal_msg_rfc8439(dummy, bytes(12), 12, None, 5, b"", 0, out) == SG_E_ARG
    assert b"NULL buffer" in lib.sg_last_error()
    assert lib.sg_open_msg_rfc8439(dummy, bytes(12), 12, bytes(15), 15, b"", 0, out) == SG_E_SHORT


def test_python_nonce_length_both_ways():
    from suruga_amd import msg

    item = lambda nonce: [msg.MsgItem(0, nonce, None, None)]
    for nonce, rfc in ((bytes(8), True), (bytes(12), False), (bytes(11), True), (bytes(16), True), (bytes(16), False)):
        with pytest.raises(ValueError, match="nonce must be"):
            msg.seal_msg(None, nonce, None, None, rfc8439=rfc)
        with pytest.raises(ValueError, match="nonce must be"):
            msg.open_(None, nonce, None, None, object(), rfc8439=rfc)
        with pytest.raises(ValueError, match="nonce must be"):
            msg.seal_msgs(None, item(nonce), rfc8439=rfc)
        with pytest.raises(ValueError, match="nonce must be"):
            msg.open_msgs(None, item(nonce), object(), rfc8439=rfc)


def test_aead_mirror_constants():
    from suruga_amd import ChaCha20Poly1305, ChaCha20Poly1305Rfc8439

    aead = ChaCha20Poly1305Rfc8439()
    assert (aead.key_size(), aead.fixed_iv_len(), aead.mac_len()) == (32, 12, 16)
    assert ChaCha20Poly1305().fixed_iv_len() == 0  # the draft's suite is as it was
    with pytest.raises(ValueError):
        aead.new_encryptor(bytes(31))
