"""The IPsec ESP packet with ChaCha20-Poly1305 restated for the tests -- TEST INFRASTRUCTURE ONLY.

RFC 7634 over RFC 4303 over tests/rfc8439_ref.py (the AEAD), written from the definition:

    be32(spi) || be32(seq_lo) || be64(iv) ||
    AEAD(key, nonce = salt || be64(iv), payload || 01 02 .. pad || u8(pad) || u8(next_header),
         AD = be32(spi) || be32(seq_lo), or with ESN be32(spi) || be32(seq_hi) || be32(seq_lo))

* ``pad_len`` / ``padded_len`` / ``packet_len``: payload, padding and the two trailer bytes
  end on a multiple of ``align``.
* ``protect``: one payload -> the packet.  Without ESN the sequence number is taken mod
  2^32, also where it stands in for the IV.
* ``unprotect``: one packet -> (status, plaintext, seq, payload_len, next_header), the
  checks in the order of include/suruga_gpu.h; the decryption always runs once the header
  is good.
* ``seq_hi``: RFC 4303 appendix A2.1 as Linux xfrm_replay_seqhi writes it; ``seq_in_window``
  is the interval definition it is held against (tests/test_esp_ref.py).

tests/golden/esp_packets.json (OpenSSL alone) ties it to an independent source.  Imports
without torch and without a GPU."""
from __future__ import annotations

import json
import struct
from pathlib import Path

import rfc8439_ref as R

GOLDEN = Path(__file__).resolve().parent / "golden" / "esp_packets.json"
HEADER_LEN, OVERHEAD, MIN_PACKET, MAX_PACKET_LEN = 16, 32, 34, 16384
OK, BAD_MAC, SHORT, SKIPPED, BAD_HEADER, BAD_INNER = 0, 1, 2, 3, 6, 7
M32 = 0xFFFFFFFF


def pad_len(n: int, align: int = 4) -> int:
    return (align - (n + 2) % align) % align


def padded_len(n: int, align: int = 4) -> int:
    return n + pad_len(n, align) + 2


def packet_len(n: int, align: int = 4) -> int:
    return OVERHEAD + padded_len(n, align)


def trailer(pad: int, next_header: int) -> bytes:
    return bytes(range(1, pad + 1)) + bytes([pad, next_header])


def nonce_of(salt: bytes, iv: int) -> bytes:
    return bytes(salt) + struct.pack(">Q", iv)


def ad_of(spi: int, seq: int, esn: bool) -> bytes:
    return struct.pack(">III", spi, seq >> 32, seq & M32) if esn else struct.pack(">II", spi, seq & M32)


def header_of(spi: int, seq: int, iv: int) -> bytes:
    return struct.pack(">IIQ", spi, seq & M32, iv)


def protect(key: bytes, salt: bytes, spi: int, seq: int, payload: bytes, next_header: int, *, align: int = 4,
            esn: bool = False, iv=None) -> bytes:
    if not esn:
        seq &= M32
    iv = seq if iv is None else iv
    pt = bytes(payload) + trailer(pad_len(len(payload), align), next_header)
    return header_of(spi, seq, iv) + R.seal(key, nonce_of(salt, iv), pt, ad_of(spi, seq, esn))


def protect_plain(key: bytes, salt: bytes, spi: int, seq: int, pt: bytes, *, esn: bool = False, iv=None) -> bytes:
    """The packet of a given AEAD plaintext, trailer and all: for the trailers no seal writes."""
    if not esn:
        seq &= M32
    iv = seq if iv is None else iv
    return header_of(spi, seq, iv) + R.seal(key, nonce_of(salt, iv), bytes(pt), ad_of(spi, seq, esn))


def seq_hi(top: int, window: int, seq_lo: int) -> int:
    th, tl = top >> 32, top & M32
    bl = (tl - window + 1) & M32
    if tl >= ((window - 1) & M32):
        return (th + 1) & M32 if seq_lo < bl else th
    return (th - 1) & M32 if seq_lo >= bl else th


def seq_in_window(top: int, window: int, seq_lo: int) -> int:
    """The one 64-bit number with the low bits seq_lo in [T - W + 1, T - W + 1 + 2^32), mod 2^64."""
    lo = top - window + 1
    return (lo + ((seq_lo - lo) & M32)) & (2**64 - 1)


def parse_trailer(pt: bytes):
    """(payload_len, next_header) of a decryption, or None where the padding is not 1 .. pad."""
    n, pad, nh = len(pt), pt[-2], pt[-1]
    if pad + 2 > n or pt[n - 2 - pad:n - 2] != bytes(range(1, pad + 1)):
        return None
    return n - 2 - pad, nh


def unprotect(key: bytes, salt: bytes, spi: int, pkt: bytes, *, esn: bool = False, top: int = 0, window: int = 0,
              want_trailer: bool = True, max_len: int = MAX_PACKET_LEN):
    """(status, plaintext, seq, payload_len, next_header).  SKIPPED, SHORT and BAD_HEADER write
    nothing: (status, None, None, None, None).  BAD_MAC comes with the decryption and the
    inferred sequence number (what SG_ESP_KEEP_FAILED leaves; without it both are zeroed) and
    payload_len and next_header 0.  Both are None where nothing is parsed (want_trailer false)."""
    if len(pkt) > max_len:
        return SKIPPED, None, None, None, None
    if len(pkt) < MIN_PACKET:
        return SHORT, None, None, None, None
    if bytes(pkt[:4]) != struct.pack(">I", spi):
        return BAD_HEADER, None, None, None, None
    lo, iv = struct.unpack(">IQ", bytes(pkt[4:16]))
    seq = (seq_hi(top, window, lo) << 32 | lo) if esn else lo
    rc, pt = R.open(key, nonce_of(salt, iv), bytes(pkt[16:]), ad_of(spi, seq, esn))
    none = (None, None) if not want_trailer else (0, 0)
    if rc:
        return BAD_MAC, pt, seq, *none
    if not want_trailer:
        return OK, pt, seq, None, None
    tr = parse_trailer(pt)
    return (OK, pt, seq, *tr) if tr is not None else (BAD_INNER, pt, seq, 0, 0)


def golden() -> dict:
    return json.loads(GOLDEN.read_text())
