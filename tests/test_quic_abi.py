"""sg_seal_batch_quic / sg_open_batch_quic reject bad arguments before any GPU work, so the
checks are pinned here on the CPU with dummy device addresses (never dereferenced), as
tests/test_abi.py does; the ctypes mirror of sg_quic_batch has the header's layout; and
the host-only helpers sg_quic_decode_pn and sg_quic_packet_keys say what tests/quic_ref.py
says.  CPU only."""
from __future__ import annotations

import ctypes as C
import random
import re

import numpy as np
import pytest

import quic_ref as Q
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def good():
    from suruga_amd._native import SgQuicBatch

    b = SgQuicBatch()
    b.count, b.flags, b.num_keys = 4, 0, 2
    b.keys, b.ivs, b.hp_keys = 0x1000, 0x2000, 0x3000
    b.pn, b.pn_out, b.status = 0x4000, 0x5000, 0x6000
    b.in_, b.out = 0x10000, 0x20000
    b.uniform_pn_off, b.uniform_len, b.in_stride, b.out_stride = 9, 1200, 1216, 1216
    return b


FIELDS = ["count", "flags", "keys", "ivs", "hp_keys", "key_index", "pn", "pn_out", "pn_off", "num_keys", "uniform_pn_off",
          "in", "in_off", "in_stride", "out", "out_off", "out_stride", "len", "uniform_len", "max_len", "status", "stream"]


def test_struct_layout_matches_the_header():
    from suruga_amd import _native as N

    text = (ROOT / "include" / "suruga_gpu.h").read_text()
    body = re.search(r"typedef struct sg_quic_batch \{(.*?)\} sg_quic_batch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == FIELDS
    assert [n.rstrip("_") for n, _ in N.SgQuicBatch._fields_] == FIELDS
    assert C.sizeof(N.SgQuicBatch) == 152 and "152 bytes" in text
    off = {n.rstrip("_"): getattr(N.SgQuicBatch, n).offset for n, _ in N.SgQuicBatch._fields_}
    assert off == {"count": 0, "flags": 4, "keys": 8, "ivs": 16, "hp_keys": 24, "key_index": 32, "pn": 40, "pn_out": 48,
                   "pn_off": 56, "num_keys": 64, "uniform_pn_off": 68, "in": 72, "in_off": 80, "in_stride": 88, "out": 96,
                   "out_off": 104, "out_stride": 112, "len": 120, "uniform_len": 128, "max_len": 132, "status": 136,
                   "stream": 144}
    for name, v in (("SG_QUIC_MAX_PACKET_LEN", 16384), ("SG_QUIC_MAX_PN_OFF", 251), ("SG_QUIC_KEY_PHASE", 1),
                    ("SG_QUIC_KEEP_FAILED", 2)):
        m = re.search(r"#define\s+%s\s+(\w+)u" % name, text)
        assert m and int(m.group(1), 0) == v == getattr(N, name)
    for sym in ("sg_seal_batch_quic", "sg_open_batch_quic", "sg_quic_decode_pn", "sg_quic_packet_keys"):
        assert sym in N.EXPORTS and re.search(r"\b%s\(" % sym, text)


@pytest.mark.parametrize("open_", (False, True))
def test_argument_errors_before_any_gpu_call(lib, open_):
    from suruga_amd._native import SG_E_ARG, SG_QUIC_KEEP_FAILED, SG_QUIC_KEY_PHASE

    call = lib.sg_open_batch_quic if open_ else lib.sg_seal_batch_quic

    def rejected(what, **fields):
        for count in (4, 0):  # the arguments are checked first, also of an empty call
            b = good()
            b.count = count
            for name, v in fields.items():
                setattr(b, name, v)
            assert call(C.byref(b)) == SG_E_ARG, (what, count)
            assert lib.sg_last_error(), what

    assert call(None) == SG_E_ARG
    rejected("unknown flags", flags=0x4)
    rejected("unknown flags beside the known", flags=SG_QUIC_KEY_PHASE | SG_QUIC_KEEP_FAILED | 0x80000000)
    for field in ("keys", "ivs", "hp_keys", "status", "in_", "out", "pn"):
        rejected(f"NULL {field}", **{field: None})
    if open_:
        rejected("open without pn_out", pn_out=None)
    for field in ("ivs", "key_index", "pn_off", "len"):
        for o in (1, 2, 3):
            rejected(f"misaligned {field}", **{field: 0x7000 + o}, max_len=1200)
    for field in ("pn", "pn_out", "in_off", "out_off"):
        for o in (1, 2, 4, 7):
            rejected(f"misaligned {field}", **{field: 0x8000 + o})
    for v in (0, 252, 0xFFFFFFFF):
        rejected(f"uniform_pn_off {v}", uniform_pn_off=v)
    limit = 16384 if open_ else 16384 - 16
    rejected("uniform_len above the packet bound", uniform_len=limit + 1)
    rejected("max_len above the packet bound", len=0x9000, max_len=limit + 1)
    rejected("num_keys 0", num_keys=0)
    rejected("odd num_keys under KEY_PHASE", flags=SG_QUIC_KEY_PHASE, num_keys=3)
    rejected("num_keys 0 under KEY_PHASE", flags=SG_QUIC_KEY_PHASE, num_keys=0)


@pytest.mark.parametrize("open_", (False, True))
def test_empty_call_launches_nothing(lib, open_):
    from suruga_amd._native import SG_QUIC_KEEP_FAILED, SG_QUIC_KEY_PHASE

    call = lib.sg_open_batch_quic if open_ else lib.sg_seal_batch_quic
    limit = 16384 if open_ else 16384 - 16
    b = good()
    b.count = 0
    assert call(C.byref(b)) == 0
    b.flags, b.uniform_len = SG_QUIC_KEY_PHASE | SG_QUIC_KEEP_FAILED, limit
    assert call(C.byref(b)) == 0
    b.len, b.max_len, b.uniform_len = 0xA000, limit, 0xFFFFFFFF  # with a length array uniform_len is not read
    b.pn_off, b.uniform_pn_off = 0xB000, 0                        # ... and with pn_off, uniform_pn_off is not
    assert call(C.byref(b)) == 0
    if not open_:
        b.pn_out = None  # seal does not read it
        assert call(C.byref(b)) == 0


def test_decode_pn_against_the_reference(lib):
    assert lib.sg_quic_decode_pn(0xA82F30EA + 1, 0x9B32, 2) == 0xA82F9B32
    rng = random.Random(9000)
    top = 2**62
    for _ in range(20000):
        pn_len = rng.randint(1, 4)
        win = 1 << (8 * pn_len)
        kind = rng.randrange(4)
        exp = (rng.randrange(3 * win) if kind == 0 else top - 1 - rng.randrange(3 * win) if kind == 1
               else rng.randrange(top))
        t = rng.choice((0, 1, win // 2 - 1, win // 2, win // 2 + 1, win - 1, rng.randrange(win)))
        assert lib.sg_quic_decode_pn(exp, t, pn_len) == Q.decode_pn(exp, t, pn_len), (exp, t, pn_len)
    # truncated is cut to 8 * pn_len bits, pn_len is taken into 1..4
    assert lib.sg_quic_decode_pn(0x12345, 0xABCD67, 1) == Q.decode_pn(0x12345, 0x67, 1)
    assert lib.sg_quic_decode_pn(0x12345, 0x67, 0) == Q.decode_pn(0x12345, 0x67, 1)
    assert lib.sg_quic_decode_pn(2**40, 0x89ABCDEF, 9) == Q.decode_pn(2**40, 0x89ABCDEF, 4)


def _keys(lib, secrets, keys=True, ivs=True, hps=True, update=0, threads=1):
    count = len(secrets)
    s = np.frombuffer(b"".join(secrets), dtype=np.uint8).copy()
    k, v, h = (np.full(count * w, 0xEE, dtype=np.uint8) for w in (32, 12, 32))
    p = lambda a, on=True: a.ctypes.data_as(C.c_void_p) if on else None  # noqa: E731
    rc = lib.sg_quic_packet_keys(count, p(s), p(k, keys), p(v, ivs), p(h, hps), update, threads)
    return rc, s.tobytes(), k.tobytes(), v.tobytes(), h.tobytes()


def test_packet_keys_a5_and_expand_label(lib):
    from suruga_amd import keysched as K
    from suruga_amd._native import SG_E_ARG

    a = Q.A5
    rc, s, k, v, h = _keys(lib, [a["secret"]])
    assert (rc, s, k, v, h) == (0, a["secret"], a["key"], a["iv"], a["hp"])
    rc, s, k, v, h = _keys(lib, [a["secret"]], hps=False, update=1)
    assert (rc, s) == (0, a["ku"]) and (k, v) == Q.packet_keys(a["ku"])[:2] and h == b"\xee" * 32
    # many rows, several threads, every table optional; against sg_hkdf_expand_label and the reference
    secrets = [bytes([i]) * 32 for i in range(37)]
    for update in (0, 1):
        want_s = [Q.next_secret(x) if update else x for x in secrets]
        for threads in (1, 3, 64):
            rc, s, k, v, h = _keys(lib, secrets, update=update, threads=threads)
            assert rc == 0 and s == b"".join(want_s)
            assert k == b"".join(K.hkdf_expand_label(x, b"quic key", b"", 32) for x in want_s)
            assert v == b"".join(K.hkdf_expand_label(x, b"quic iv", b"", 12) for x in want_s)
            assert h == b"".join(K.hkdf_expand_label(x, b"quic hp", b"", 32) for x in want_s)
            assert (k[:32], v[:12], h[:32]) == Q.packet_keys(want_s[0])
    rc, s, k, v, h = _keys(lib, secrets, keys=False, hps=False)
    assert rc == 0 and k == b"\xee" * len(k) and h == b"\xee" * len(h) and v[:12] == Q.packet_keys(secrets[0])[1]
    # the rules of sg_tls13_traffic_keys
    assert lib.sg_quic_packet_keys(0, None, None, None, None, 0, 1) == 0
    assert lib.sg_quic_packet_keys(2, None, None, None, None, 1, 1) == SG_E_ARG
    assert _keys(lib, secrets, keys=False, ivs=False, hps=False)[0] == SG_E_ARG
    assert _keys(lib, secrets, keys=False, ivs=False, hps=False, update=1, threads=0)[0] == 0  # an update alone is a call
    # ... and the Python form
    keys, ivs, hps = K.quic_packet_keys(np.frombuffer(a["secret"], dtype=np.uint8).reshape(1, 32))
    assert (keys.tobytes(), ivs.tobytes(), hps.tobytes()) == (a["key"], a["iv"], a["hp"])
    keys, ivs, nxt = K.quic_packet_keys(np.frombuffer(a["secret"], dtype=np.uint8).reshape(1, 32), update=True)
    assert nxt.tobytes() == a["ku"] and (keys.tobytes(), ivs.tobytes()) == Q.packet_keys(a["ku"])[:2]


def test_python_decode_pn(lib):
    import suruga_amd

    assert suruga_amd.decode_pn(0xA82F30EA + 1, 0x9B32, 2) == 0xA82F9B32
    assert {"QuicBatch", "seal_quic", "open_quic", "decode_pn", "quic_packet_keys"} <= set(suruga_amd.__all__)


def test_kernel_file_is_part_of_the_build_and_the_source_hash():
    from suruga_amd import _build

    names = [p.name for p in _build.HIP_SOURCES]
    assert {"sg_quic.hip", "sg_quic_capi.cpp", "sg_quic_host.cpp"} <= set(names)
    assert "sg_quic.h" in [p.name for p in _build.HIP_DEPS]
