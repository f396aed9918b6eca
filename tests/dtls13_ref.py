"""The DTLS 1.3 record with TLS_CHACHA20_POLY1305_SHA256 restated for the tests -- TEST INFRASTRUCTURE ONLY.

RFC 9147 section 4 over tests/rfc8439_ref.py (the AEAD and the ChaCha20 block), written from
the definition:

    0 0 1 C S L E E || cid || seq (low 8 or 16 bits, big-endian) || [be16(|encrypted_record|)] ||
    AEAD(key, nonce = iv XOR (00 00 00 00 || be64(seq)), content || u8(type) || zeros, AD = that header)

with the sequence number bytes XORed last with the first bytes of the ChaCha20 block under
sn_key whose counter and nonce are the first 16 bytes of the encrypted record (section 4.2.3).

* ``header_len`` / ``inner_len`` / ``record_len``: the lengths, the padding capped at 2^14 + 1.
* ``protect``: one content -> the record.  ``protect_inner`` takes the whole inner plaintext
  instead, for the inner plaintexts no seal writes (all zero, empty).
* ``unprotect``: one record -> (status, inner plaintext, seq, epoch bits, content_len, type),
  the checks in the order of include/suruga_gpu.h; ``rows(ee)`` gives the (key, iv, sn_key,
  expected) the epoch bits name.
* ``decode_seq``: section 4.2.2 -- the number closest to ``expected`` with the given low bits --
  as RFC 9000 appendix A.3 computes it, and ``closest`` the definition it is held against.
* ``expand_label`` / ``record_keys``: section 5.9's labels with the prefix "dtls13".

tests/golden/dtls13_records.json (OpenSSL alone) and dtls13_keys.json (hashlib's HMAC alone)
tie it to independent sources.  Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
import hmac
import json
import struct
from pathlib import Path

import rfc8439_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "dtls13_records.json"
GOLDEN_KEYS = Path(__file__).resolve().parent / "golden" / "dtls13_keys.json"
MAX_CONTENT_LEN, MAX_CID_LEN, MAX_INNER = 16384, 250, 16385
MAX_RECORD_LEN = 255 + 16384 + 1 + 16
OK, BAD_MAC, SHORT, SKIPPED, NO_TYPE, BAD_HEADER = 0, 1, 2, 3, 5, 6
FIXED, C_BIT, S_BIT, L_BIT = 0x20, 0x10, 0x08, 0x04
SAMPLE_LEN = 16


def first_byte(seq16: bool, length: bool, cid_len: int, epoch: int) -> int:
    return FIXED | (C_BIT if cid_len else 0) | (S_BIT if seq16 else 0) | (L_BIT if length else 0) | (epoch & 3)


def header_len(seq16: bool, length: bool, cid_len: int) -> int:
    return 1 + cid_len + (2 if seq16 else 1) + (2 if length else 0)


def inner_len(n: int, pad_to: int = 0) -> int:
    base = n + 1
    if pad_to <= 1 or base >= MAX_INNER:
        return base
    return min(-(-base // pad_to) * pad_to, MAX_INNER)


def record_len(n: int, pad_to: int, seq16: bool, length: bool, cid_len: int) -> int:
    return header_len(seq16, length, cid_len) + inner_len(n, pad_to) + 16


def inner_of(content: bytes, ctype: int, pad_to: int = 0) -> bytes:
    return bytes(content) + bytes([ctype]) + bytes(inner_len(len(content), pad_to) - len(content) - 1)


def header_of(seq16: bool, length: bool, cid: bytes, epoch: int, seq: int, enc_len: int) -> bytes:
    sn = 2 if seq16 else 1
    return (bytes([first_byte(seq16, length, len(cid), epoch)]) + bytes(cid) + (seq & ((1 << (8 * sn)) - 1)).to_bytes(sn, "big")
            + (struct.pack(">H", enc_len) if length else b""))


def nonce_of(iv: bytes, seq: int) -> bytes:
    return bytes(a ^ b for a, b in zip(iv, seq.to_bytes(12, "big")))


def sn_mask(sn_key: bytes, sample: bytes) -> bytes:
    assert len(sn_key) == 32 and len(sample) == SAMPLE_LEN
    return R.chacha20_blocks(sn_key, sample[4:], int.from_bytes(sample[:4], "little"), 1).tobytes()[:2]


def apply_mask(sn_key: bytes, rec: bytes, cid_len: int) -> bytes:
    """Record number encryption over header || encrypted_record; its own inverse."""
    rec = bytearray(rec)
    hl = header_len(bool(rec[0] & S_BIT), bool(rec[0] & L_BIT), cid_len)
    mask = sn_mask(sn_key, bytes(rec[hl:hl + SAMPLE_LEN]))
    for j in range(2 if rec[0] & S_BIT else 1):
        rec[1 + cid_len + j] ^= mask[j]
    return bytes(rec)


def protect_inner(key: bytes, iv: bytes, sn_key: bytes, seq: int, inner: bytes, *, epoch: int = 0, cid: bytes = b"",
                  seq16: bool = False, length: bool = False) -> bytes:
    header = header_of(seq16, length, cid, epoch, seq, len(inner) + 16)
    return apply_mask(sn_key, header + R.seal(key, nonce_of(iv, seq), bytes(inner), header), len(cid))


def protect(key: bytes, iv: bytes, sn_key: bytes, seq: int, content: bytes, ctype: int, *, pad_to: int = 0, **form) -> bytes:
    return protect_inner(key, iv, sn_key, seq, inner_of(content, ctype, pad_to), **form)


def decode_seq(expected: int, truncated: int, nbytes: int) -> int:
    """RFC 9000 appendix A.3 with largest = expected - 1, as sg_quic_decode_pn states it."""
    win = 1 << (8 * nbytes)
    hwin, mask = win // 2, win - 1
    cand = (expected & ~mask) | (truncated & mask)
    if cand <= expected - hwin and cand < (1 << 62) - win:
        return cand + win
    if cand > expected + hwin and cand >= win:
        return cand - win
    return cand


def closest(expected: int, truncated: int, nbytes: int) -> int:
    """Section 4.2.2 by its definition: of the numbers >= 0 with these low bits, the one in
    (expected - hwin, expected + hwin], and where there is none (near zero) the closest."""
    win = 1 << (8 * nbytes)
    base = (expected & ~(win - 1)) | (truncated & (win - 1))
    cands = [c for c in (base - win, base, base + win) if c >= 0]
    inside = [c for c in cands if expected - win // 2 < c <= expected + win // 2]
    return inside[0] if inside else min(cands, key=lambda c: abs(c - expected))


def strip(inner: bytes):
    """(content_len, type) of an inner plaintext, or None where it has no non-zero byte."""
    i = len(inner)
    while i and inner[i - 1] == 0:
        i -= 1
    return (i - 1, inner[i - 1]) if i else None


def unprotect(rows, rec: bytes, cid_len: int, *, max_len: int = MAX_RECORD_LEN):
    """(status, inner, seq, ee, content_len, type).  rows(ee) -> (key, iv, sn_key, expected).
    SKIPPED, SHORT and BAD_HEADER write nothing: (status, None, None, None, None, None).
    BAD_MAC comes with the decryption and the decoded sequence number (what
    SG_DTLS13_KEEP_FAILED leaves; without it both are zeroed) and content_len and type 0."""
    nothing = (None,) * 5
    if len(rec) > max_len:
        return SKIPPED, *nothing
    if len(rec) == 0:
        return SHORT, *nothing
    b0 = rec[0]
    if b0 & 0xE0 != FIXED or bool(b0 & C_BIT) != bool(cid_len):
        return BAD_HEADER, *nothing
    seq16, length = bool(b0 & S_BIT), bool(b0 & L_BIT)
    hl = header_len(seq16, length, cid_len)
    if len(rec) < hl + 16:
        return SHORT, *nothing
    if length and struct.unpack(">H", bytes(rec[hl - 2:hl]))[0] != len(rec) - hl:
        return BAD_HEADER, *nothing
    ee = b0 & 3
    key, iv, sn_key, expected = rows(ee)
    clear = apply_mask(sn_key, rec, cid_len)
    sn = 2 if seq16 else 1
    seq = decode_seq(expected, int.from_bytes(clear[1 + cid_len:1 + cid_len + sn], "big"), sn)
    rc, inner = R.open(key, nonce_of(iv, seq), clear[hl:], clear[:hl])
    if rc:
        return BAD_MAC, inner, seq, ee, 0, 0
    st = strip(inner)
    return (OK, inner, seq, ee, *st) if st is not None else (NO_TYPE, inner, seq, ee, 0, 0)


# ---- keys (RFC 9147 section 5.9 over RFC 8446 section 7.1)
def expand_label(secret: bytes, label: bytes, context: bytes, length: int) -> bytes:
    full = b"dtls13" + label
    info = struct.pack(">H", length) + bytes([len(full)]) + full + bytes([len(context)]) + context
    out, t, i = b"", b"", 1
    while len(out) < length:
        t = hmac.new(secret, t + info + bytes([i]), hashlib.sha256).digest()
        out, i = out + t, i + 1
    return out[:length]


def record_keys(secret: bytes):
    """(key, iv, sn_key) of a traffic secret."""
    return expand_label(secret, b"key", b"", 32), expand_label(secret, b"iv", b"", 12), expand_label(secret, b"sn", b"", 32)


def next_secret(secret: bytes) -> bytes:
    return expand_label(secret, b"traffic upd", b"", 32)


def golden() -> dict:
    return json.loads(GOLDEN.read_text())


def golden_keys() -> dict:
    return json.loads(GOLDEN_KEYS.read_text())
