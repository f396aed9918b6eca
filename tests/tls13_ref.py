"""TLS 1.3 record protection restated for the tests -- TEST INFRASTRUCTURE ONLY.

RFC 8446 section 5.2 - 5.4 over tests/rfc8439_ref.py (imported, not edited):

* ``nonce``: the write IV XOR the sequence number, left-padded to 12 bytes (5.3).
* ``header``: the record header 17 03 03 be16(L), which is the additional data (5.2).
* ``inner``: TLSInnerPlaintext = content || type || zeros (5.2, 5.4).
* ``seal``: the fragment ct(inner) || tag.
* ``open``: (status, inner bytes, inner type, content length) as the record batch
  reports them: 2 for a fragment below 16 bytes, 1 for a wrong tag, 5 where the tag is
  good and the inner plaintext holds no non-zero byte, else 0 with the type and length.
* ``strip``: the last non-zero byte and the number of bytes before it.

Imports without torch and without a GPU."""
from __future__ import annotations

import struct

import rfc8439_ref as R

OK, BAD_MAC, SHORT, NO_TYPE = 0, 1, 2, 5
APPLICATION_DATA = 23
MAX_CONTENT = 1 << 14
MAX_FRAGMENT = (1 << 14) + 256


def nonce(iv12: bytes, seq: int) -> bytes:
    assert len(iv12) == 12 and 0 <= seq < 1 << 64
    return bytes(a ^ b for a, b in zip(iv12, bytes(4) + struct.pack(">Q", seq)))


def header(frag_len: int) -> bytes:
    return struct.pack(">BBBH", 23, 3, 3, frag_len)


def inner(content: bytes, ctype: int, pad: int = 0) -> bytes:
    assert 0 < ctype < 256
    return bytes(content) + bytes([ctype]) + bytes(pad)


def seal_inner(key: bytes, iv12: bytes, seq: int, inner_pt: bytes) -> bytes:
    """The fragment of any inner plaintext (an all-zero one too, which no sender builds)."""
    return R.seal(key, nonce(iv12, seq), inner_pt, header(len(inner_pt) + 16))


def seal(key: bytes, iv12: bytes, seq: int, content: bytes, ctype: int = APPLICATION_DATA, pad: int = 0) -> bytes:
    return seal_inner(key, iv12, seq, inner(content, ctype, pad))


def strip(inner_pt: bytes):
    """(type, content length), or None where every byte is zero."""
    k = len(inner_pt)
    while k and inner_pt[k - 1] == 0:
        k -= 1
    return (inner_pt[k - 1], k - 1) if k else None


def open(key: bytes, iv12: bytes, seq: int, frag: bytes):  # noqa: A001  (the checker's name for it)
    """(status, inner, type, content_len); the inner bytes are the decryption, which
    always runs (nothing for a fragment below 16 bytes)."""
    rc, pt = R.open(key, nonce(iv12, seq), frag, header(len(frag)))
    if rc:
        return rc, pt, 0, 0
    s = strip(pt)
    if s is None:
        return NO_TYPE, pt, 0, 0
    return OK, pt, s[0], s[1]
