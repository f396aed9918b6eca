"""The WireGuard transport data message restated for the tests -- TEST INFRASTRUCTURE ONLY.

Whitepaper section 5.4.6 over tests/rfc8439_ref.py (the AEAD), written from the definition:

    le32(4) || le32(receiver) || le64(counter) ||
    AEAD(key, nonce = 00 00 00 00 || le64(counter), inner || zeros, AD = empty)

* ``padded_len`` / ``message_len``: the inner packet rounded up to 16, at most
  max(len, pad_cap) where there is a pad_cap (Linux: min(MTU, ALIGN(len, 16))).
* ``protect``: one inner packet -> the message.
* ``unprotect``: one message -> (status, plaintext, counter, inner_len), the checks in
  the order of include/suruga_gpu.h; the decryption always runs once the header is good.
* ``inner_len_of``: the inner packet's length from its IPv4 / IPv6 header, None where it
  does not fit.

tests/golden/wg_packets.json (OpenSSL alone) ties it to an independent source
(tests/test_wg_ref.py).  Imports without torch and without a GPU."""
from __future__ import annotations

import json
import struct
from pathlib import Path

import rfc8439_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "wg_packets.json"
HEADER_LEN, OVERHEAD, MAX_MESSAGE_LEN = 16, 32, 16384
OK, BAD_MAC, SHORT, SKIPPED, BAD_HEADER, BAD_INNER = 0, 1, 2, 3, 6, 7
REJECT_AFTER_MESSAGES = 2**64 - 2**13 - 1


def padded_len(n: int, pad_cap: int = 0) -> int:
    up = (n + 15) // 16 * 16
    return min(up, max(n, pad_cap)) if pad_cap else up


def message_len(n: int, pad_cap: int = 0) -> int:
    return OVERHEAD + padded_len(n, pad_cap)


def nonce_of(counter: int) -> bytes:
    return bytes(4) + struct.pack("<Q", counter)


def header_of(receiver: int, counter: int) -> bytes:
    return struct.pack("<IIQ", 4, receiver, counter)


def protect(key: bytes, receiver: int, counter: int, inner: bytes, pad_cap: int = 0) -> bytes:
    pt = bytes(inner) + bytes(padded_len(len(inner), pad_cap) - len(inner))
    return header_of(receiver, counter) + R.seal(key, nonce_of(counter), pt, b"")


def be16(b: bytes) -> int:
    return (b[0] << 8) | b[1]


def inner_len_of(pt: bytes):
    """The length the IP header of `pt` (a non-empty decryption) states, or None."""
    n, ver = len(pt), pt[0] >> 4
    if ver == 4 and n >= 20:
        L = be16(pt[2:4])
        return L if 20 <= L <= n else None
    if ver == 6 and n >= 40:
        L = 40 + be16(pt[4:6])
        return L if L <= n else None
    return None


def unprotect(key: bytes, msg: bytes, want_inner_len: bool = True, max_len: int = MAX_MESSAGE_LEN):
    """(status, plaintext, counter, inner_len).  SKIPPED, SHORT and BAD_HEADER write nothing:
    (status, None, None, None).  BAD_MAC comes with the decryption and the wire counter (what
    SG_WG_KEEP_FAILED leaves; without it both are zeroed) and inner_len 0.  inner_len is None
    where nothing is parsed (want_inner_len false)."""
    if len(msg) > max_len:
        return SKIPPED, None, None, None
    if len(msg) < OVERHEAD:
        return SHORT, None, None, None
    if bytes(msg[:4]) != b"\x04\0\0\0":
        return BAD_HEADER, None, None, None
    counter = struct.unpack("<Q", bytes(msg[8:16]))[0]
    rc, pt = R.open(key, nonce_of(counter), bytes(msg[16:]), b"")
    if rc:
        return BAD_MAC, pt, counter, (0 if want_inner_len else None)
    if not want_inner_len:
        return OK, pt, counter, None
    if not pt:
        return OK, pt, counter, 0
    L = inner_len_of(pt)
    return (OK, pt, counter, L) if L is not None else (BAD_INNER, pt, counter, 0)


def ipv4(total: int, n: int, what: str = "v4") -> bytes:
    """n bytes that start with an IPv4 header stating `total`."""
    b = bytearray(R.data(n, b"wg inner " + what.encode() + b" %d %d" % (total, n)))
    b[0] = 0x45
    if n >= 4:
        b[2:4] = struct.pack(">H", total & 0xFFFF)
    return bytes(b)


def ipv6(payload: int, n: int, what: str = "v6") -> bytes:
    """n bytes that start with an IPv6 header stating a payload length."""
    b = bytearray(R.data(n, b"wg inner " + what.encode() + b" %d %d" % (payload, n)))
    b[0] = 0x60 | (b[0] & 0x0F)
    if n >= 6:
        b[4:6] = struct.pack(">H", payload & 0xFFFF)
    return bytes(b)


def golden() -> dict:
    return json.loads(GOLDEN.read_text())
