"""HKDF and the TLS 1.3 traffic keys restated for the tests -- TEST INFRASTRUCTURE ONLY.

RFC 5869 with SHA-256 and RFC 8446 section 7.1 - 7.3 over Python's ``hmac`` /
``hashlib``, written from the RFCs' definitions:

* ``extract``: HKDF-Extract(salt, IKM) = HMAC(salt, IKM); no salt is 32 zero bytes.
* ``expand``: HKDF-Expand(PRK, info, L): T(0) = "", T(i) = HMAC(PRK, T(i-1) || info || i).
* ``hkdf_label`` / ``expand_label``: HkdfLabel = be16(L) || u8(6 + |label|) || "tls13 " ||
  label || u8(|context|) || context, and HKDF-Expand over it.
* ``traffic_keys``: key = Expand-Label(secret, "key", "", 32), iv = Expand-Label(secret, "iv", "", 12).
* ``next_secret``: Expand-Label(secret, "traffic upd", "", 32), the KeyUpdate ratchet.

tests/golden/tls13_keys.json (OpenSSL's TLS13-KDF) ties it to an independent
implementation (tests/test_tls13_keys_ref.py).  Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
import hmac
import struct

HASH_LEN = 32
KEY_LEN, IV_LEN = 32, 12


def extract(salt: bytes, ikm: bytes) -> bytes:
    return hmac.new(salt if salt else bytes(HASH_LEN), ikm, hashlib.sha256).digest()


def expand(prk: bytes, info: bytes, length: int) -> bytes:
    assert 0 <= length <= 255 * HASH_LEN
    t, okm, i = b"", b"", 1
    while len(okm) < length:
        t = hmac.new(prk, t + info + bytes([i]), hashlib.sha256).digest()
        okm += t
        i += 1
    return okm[:length]


def hkdf_label(length: int, label: bytes, context: bytes) -> bytes:
    assert len(label) <= 249 and len(context) <= 255 and length < 1 << 16
    full = b"tls13 " + label
    return struct.pack(">HB", length, len(full)) + full + bytes([len(context)]) + context


def expand_label(secret: bytes, label: bytes, context: bytes, length: int) -> bytes:
    return expand(secret, hkdf_label(length, label, context), length)


def traffic_keys(secret: bytes):
    """(key, iv) of a traffic secret (RFC 8446 section 7.3)."""
    return expand_label(secret, b"key", b"", KEY_LEN), expand_label(secret, b"iv", b"", IV_LEN)


def next_secret(secret: bytes) -> bytes:
    """application_traffic_secret_N+1 (RFC 8446 section 7.2)."""
    return expand_label(secret, b"traffic upd", b"", HASH_LEN)


def generation(secret: bytes, n: int) -> bytes:
    for _ in range(n):
        secret = next_secret(secret)
    return secret


def secrets(count: int, tag: bytes = b"tls13 traffic secrets") -> list:
    """count secrets for the tests: row 0 all zero, row 1 all ff (where there are that
    many), the rest SHAKE-256 of the tag with the high bit of every row's first byte set."""
    raw = hashlib.shake_256(tag + b" %d" % count).digest(32 * count)
    rows = [bytearray(raw[32 * i:32 * i + 32]) for i in range(count)]
    for r in rows:
        r[0] |= 0x80
    rows[0][:] = bytes(32)
    if count > 1:
        rows[1][:] = b"\xff" * 32
    return [bytes(r) for r in rows]
