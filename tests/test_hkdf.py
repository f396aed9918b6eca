"""The host HKDF calls (sg_keysched.cpp: sg_hkdf_extract, sg_hkdf_expand_label,
sg_tls13_traffic_keys) against tests/tls13_keys_ref.py and OpenSSL's bytes
(tests/golden/tls13_keys.json), through the C ABI and through suruga_amd.keysched.
All comparisons are byte equality.  CPU only."""
from __future__ import annotations

import ctypes as C
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import tls13_keys_ref as R

DOC = json.loads((Path(__file__).resolve().parent / "golden" / "tls13_keys.json").read_text())
SECRET = hashlib.sha256(b"hkdf test secret").digest()


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def expand_label(lib, secret, label, context, n, room=None):
    size = (n if room is None else room) + 8
    out = C.create_string_buffer(b"\xa5" * size, size)  # exactly size bytes: no terminator behind them
    rc = lib.sg_hkdf_expand_label(secret, label or None, len(label), context or None, len(context), out, n)
    return rc, out.raw


def data(n: int, tag: bytes) -> bytes:
    return hashlib.shake_256(tag).digest(n) if n else b""


OUT_LENS = (0, 1, 31, 32, 33, 64, 8160)
LABEL_LENS = (0, 1, 11, 249)
CONTEXT_LENS = (0, 32, 255)


@pytest.mark.parametrize("label_len", LABEL_LENS)
@pytest.mark.parametrize("context_len", CONTEXT_LENS)
def test_expand_label_against_reference(lib, label_len, context_len):
    label, context = data(label_len, b"label"), data(context_len, b"context")
    for n in OUT_LENS:
        rc, raw = expand_label(lib, SECRET, label, context, n)
        assert rc == 0, (n, lib.sg_last_error())
        assert raw[:n] == R.expand_label(SECRET, label, context, n), (label_len, context_len, n)
        assert raw[n:] == b"\xa5" * 8, "bytes behind out_len were written"


def test_info_crossing_a_block(lib):
    """The inner hash's message is T(i-1) || info || i behind the 64-byte key block.  With
    info of 54 bytes T(1)'s message still leaves room for SHA-256's padding in its block,
    with 55 (55 + 1 + 1 + 8 > 64) it no longer does, and 63 .. 65 cross the block itself;
    T(2) and T(3) carry 32 more bytes in front, so every one of them crosses."""
    for info_len in (54, 55, 56, 63, 64, 65):
        label = data(info_len - 10 - 32, b"crossing")  # info = 2 + 1 + 6 + label + 1 + 32 context bytes
        context = data(32, b"ctx")
        assert len(R.hkdf_label(96, label, context)) == info_len
        rc, raw = expand_label(lib, SECRET, label, context, 96)
        assert rc == 0 and raw[:96] == R.expand_label(SECRET, label, context, 96), info_len


def test_expand_label_bounds(lib):
    from suruga_amd._native import SG_E_ARG

    for label_len, context_len, n in ((249, 255, 8161), (250, 0, 32), (0, 256, 32)):
        rc, raw = expand_label(lib, SECRET, bytes(label_len), bytes(context_len), n, room=16)
        assert rc == SG_E_ARG and lib.sg_last_error(), (label_len, context_len, n)
        assert raw == b"\xa5" * 24
    assert expand_label(lib, SECRET, bytes(249), bytes(255), 8160)[0] == 0
    out = C.create_string_buffer(32)
    assert lib.sg_hkdf_expand_label(None, b"key", 3, None, 0, out, 32) == SG_E_ARG
    assert lib.sg_hkdf_expand_label(SECRET, None, 3, None, 0, out, 32) == SG_E_ARG
    assert lib.sg_hkdf_expand_label(SECRET, b"key", 3, None, 1, out, 32) == SG_E_ARG
    assert lib.sg_hkdf_expand_label(SECRET, b"key", 3, None, 0, None, 32) == SG_E_ARG
    assert lib.sg_hkdf_expand_label(SECRET, b"key", 3, None, 0, None, 0) == 0  # out_len 0 writes nothing


def test_extract(lib):
    from suruga_amd._native import SG_E_ARG

    def extract(salt, salt_len, ikm):
        out = C.create_string_buffer(32)
        return lib.sg_hkdf_extract(salt, salt_len, ikm or None, len(ikm), out), out.raw

    ikm = data(48, b"ikm")
    assert extract(None, 0, ikm) == (0, R.extract(b"", ikm))
    assert extract(bytes(32), 32, ikm) == (0, R.extract(b"", ikm))  # no salt = 32 zero bytes
    salt = data(32, b"salt")
    assert extract(salt, 32, ikm) == (0, R.extract(salt, ikm))
    assert extract(salt, 32, b"") == (0, R.extract(salt, b""))
    assert extract(None, 0, b"") == (0, R.extract(b"", b""))
    assert extract(data(64, b"s64"), 64, ikm) == (0, R.extract(data(64, b"s64"), ikm))
    assert extract(data(65, b"s65"), 65, ikm)[0] == SG_E_ARG and b"64" in lib.sg_last_error()
    assert extract(None, 5, ikm)[0] == SG_E_ARG
    assert lib.sg_hkdf_extract(None, 0, None, 3, C.create_string_buffer(32)) == SG_E_ARG
    assert lib.sg_hkdf_extract(None, 0, None, 0, None) == SG_E_ARG
    # RFC 5869 A.1
    assert extract(bytes(range(13)), 13, bytes([0x0B] * 22))[1].hex() == \
        "077709362c2e32df0ddc3f0dc47bba6390b6c73bb50f9c3122ec844ad7c2b3e5"


def traffic(lib, secrets, update, threads, keys=True, ivs=True):
    """sg_tls13_traffic_keys over exact-size tables in sentinel-framed buffers: (rc, secrets, keys, ivs)."""
    count = len(secrets)
    frame = lambda body: C.create_string_buffer(b"\x5a" * 8 + body + b"\x5a" * 8, len(body) + 16)  # noqa: E731
    s, k, v = frame(b"".join(secrets)), frame(b"\xa5" * 32 * count), frame(b"\xa5" * 12 * count)
    at = lambda b: C.c_void_p(C.addressof(b) + 8)  # noqa: E731
    rc = lib.sg_tls13_traffic_keys(count, at(s), at(k) if keys else None, at(v) if ivs else None, update, threads)
    for b in (s, k, v):
        assert b.raw[:8] == b"\x5a" * 8 and b.raw[-8:] == b"\x5a" * 8, "a byte outside the tables was written"
    return rc, s.raw[8:8 + 32 * count], k.raw[8:8 + 32 * count], v.raw[8:8 + 12 * count]


@pytest.mark.parametrize("count", (0, 1, 5))
@pytest.mark.parametrize("threads", (1, 3))
@pytest.mark.parametrize("update", (0, 1))
def test_traffic_keys_against_reference(lib, count, threads, update):
    secrets = R.secrets(count) if count else []
    then = [R.next_secret(s) if update else s for s in secrets]
    want_k = b"".join(R.traffic_keys(s)[0] for s in then)
    want_v = b"".join(R.traffic_keys(s)[1] for s in then)
    assert traffic(lib, secrets, update, threads) == (0, b"".join(then), want_k, want_v)
    if count:  # NULL keys / NULL ivs: the other table alone, the absent one untouched
        assert traffic(lib, secrets, update, threads, keys=False) == (0, b"".join(then), b"\xa5" * 32 * count, want_v)
        assert traffic(lib, secrets, update, threads, ivs=False) == (0, b"".join(then), want_k, b"\xa5" * 12 * count)


def test_traffic_keys_arguments(lib):
    from suruga_amd._native import SG_E_ARG

    secrets = R.secrets(2)
    assert traffic(lib, secrets, 0, 1, keys=False, ivs=False)[0] == SG_E_ARG and lib.sg_last_error()
    rc, s, k, v = traffic(lib, secrets, 1, 1, keys=False, ivs=False)  # an update alone ratchets
    assert (rc, s) == (0, b"".join(R.next_secret(x) for x in secrets)) and k == b"\xa5" * 64 and v == b"\xa5" * 24
    out = C.create_string_buffer(64)
    assert lib.sg_tls13_traffic_keys(2, None, out, None, 0, 1) == SG_E_ARG
    assert lib.sg_tls13_traffic_keys(0, None, None, None, 0, 1) == 0
    assert traffic(lib, secrets, 0, 0)[0] == 0 and traffic(lib, secrets, 0, 64)[0] == 0  # threads are clamped to 1..count


def test_three_updates_equal_the_reference_chain(lib):
    secrets = R.secrets(5)
    cur = secrets
    for g in range(1, 4):
        rc, s, k, v = traffic(lib, cur, 1, 3)
        cur = [s[32 * i:32 * i + 32] for i in range(5)]
        assert rc == 0 and cur == [R.generation(x, g) for x in secrets], g
        assert k == b"".join(R.traffic_keys(x)[0] for x in cur) and v == b"".join(R.traffic_keys(x)[1] for x in cur)


def test_fixture_bytes(lib):
    secrets = [bytes.fromhex(c["secret"]) for c in DOC["cases"]]
    rc, _, k, v = traffic(lib, secrets, 0, 2)
    assert rc == 0 and k.hex() == "".join(c["key"] for c in DOC["cases"]) and v.hex() == "".join(c["iv"] for c in DOC["cases"])
    rc, s, _, _ = traffic(lib, secrets, 1, 2)
    assert rc == 0 and s.hex() == "".join(c["traffic upd"] for c in DOC["cases"])
    for c in DOC["cases"]:
        for label, n in DOC["labels"].items():
            assert expand_label(lib, bytes.fromhex(c["secret"]), label.encode(), b"", n)[1][:n].hex() == c[label]
    cur = [bytes.fromhex(DOC["chain"][0]["secret"])]
    for c in DOC["chain"][1:]:
        rc, s, k, v = traffic(lib, cur, 1, 1)
        assert (rc, s.hex(), k.hex(), v.hex()) == (0, c["secret"], c["key"], c["iv"])
        cur = [s]


def test_python_wrappers(lib):
    from suruga_amd import keysched as K

    assert K.hkdf_extract(b"", b"ikm") == R.extract(b"", b"ikm") == K.hkdf_extract(None, b"ikm")
    assert K.hkdf_expand_label(SECRET, b"finished", b"", 32) == R.expand_label(SECRET, b"finished", b"", 32)
    assert K.hkdf_expand_label(SECRET, b"exp master", SECRET, 0) == b""
    with pytest.raises(ValueError):
        K.hkdf_expand_label(bytes(31), b"key", b"", 32)
    secrets = R.secrets(5)
    arr = np.frombuffer(b"".join(secrets), dtype=np.uint8).reshape(5, 32)
    keys, ivs = K.tls13_traffic_keys(arr, threads=2)
    assert keys.shape == (5, 32) and ivs.shape == (5, 12) and keys.dtype == ivs.dtype == np.uint8
    assert [bytes(k) for k in keys] == [R.traffic_keys(s)[0] for s in secrets]
    assert [bytes(v) for v in ivs] == [R.traffic_keys(s)[1] for s in secrets]
    keys, ivs, nxt = K.tls13_traffic_keys(arr, update=True)
    assert [bytes(s) for s in nxt] == [R.next_secret(s) for s in secrets]
    assert [bytes(k) for k in keys] == [R.traffic_keys(R.next_secret(s))[0] for s in secrets]
    assert arr.tobytes() == b"".join(secrets), "the caller's secrets were ratcheted in place"
    with pytest.raises(ValueError):
        K.tls13_traffic_keys(np.zeros((2, 31), dtype=np.uint8))
