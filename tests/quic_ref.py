"""QUIC packet protection restated for the tests -- TEST INFRASTRUCTURE ONLY.

RFC 9001 section 5.3 - 5.4 and RFC 9000 appendix A.3 over tests/rfc8439_ref.py (the AEAD
and the ChaCha20 block) and tests/tls13_keys_ref.py (HKDF-Expand-Label), written from the
RFCs' definitions:

* ``hp_mask``: the first 5 bytes of the ChaCha20 block under the header protection key
  with counter le32(sample[0..4)) and nonce sample[4..16)  (section 5.4.4).
* ``protect`` / ``unprotect``: one packet, header || payload <-> protected packet.
* ``decode_pn``: appendix A.3 in Python integers, expected_pn = largest_pn + 1.
* ``packet_keys`` / ``next_secret``: "quic key", "quic iv", "quic hp", "quic ku".

tests/golden/quic_packets.json (OpenSSL alone) and RFC 9001 appendix A.5 tie it to
independent sources (tests/test_quic_ref.py).  Imports without torch and without a GPU."""
from __future__ import annotations

import json
from pathlib import Path

import rfc8439_ref as R
import tls13_keys_ref as H

GOLDEN = Path(__file__).resolve().parent / "golden" / "quic_packets.json"
SAMPLE_LEN = 16

# RFC 9001 appendix A.5
A5 = {
    "secret": bytes.fromhex("9ac312a7f877468ebe69422748ad00a15443f18203a07d6060f688f30f21632b"),
    "key": bytes.fromhex("c6d98ff3441c3fe1b2182094f69caa2ed4b716b65488960a7a984979fb23e1c8"),
    "iv": bytes.fromhex("e0459b3474bdd0e44a41c144"),
    "hp": bytes.fromhex("25a282b9e82f06f21f488917a4fc8f1b73573685608597d0efcb076b0ab7a7a4"),
    "ku": bytes.fromhex("1223504755036d556342ee9361d253421a826c9ecdf3c7148684b36b714881f9"),
    "pn": 654360564,
    "header": bytes.fromhex("4200bff4"),
    "payload": bytes.fromhex("01"),
    "sample": bytes.fromhex("5e5cd55c41f69080575d7999c25a5bfb"),
    "mask": bytes.fromhex("aefefe7d03"),
    "packet": bytes.fromhex("4cfe4189655e5cd55c41f69080575d7999c25a5bfb"),
}


def packet_keys(secret: bytes):
    """(key, iv, hp) of a packet protection secret (RFC 9001 section 5.1)."""
    return (H.expand_label(secret, b"quic key", b"", 32), H.expand_label(secret, b"quic iv", b"", 12),
            H.expand_label(secret, b"quic hp", b"", 32))


def next_secret(secret: bytes) -> bytes:
    """The next generation's secret (RFC 9001 section 6.1)."""
    return H.expand_label(secret, b"quic ku", b"", 32)


def hp_mask(hp: bytes, sample: bytes) -> bytes:
    assert len(hp) == 32 and len(sample) == SAMPLE_LEN
    return R.chacha20_blocks(hp, sample[4:], int.from_bytes(sample[:4], "little"), 1).tobytes()[:5]


def nonce_of(iv: bytes, pn: int) -> bytes:
    return bytes(a ^ b for a, b in zip(iv, pn.to_bytes(12, "big")))


def first_byte_bits(b0: int) -> int:
    return 0x0F if b0 & 0x80 else 0x1F


def pn_len_of(b0: int) -> int:
    return (b0 & 3) + 1


def header_of(raw: bytes, pn_off: int, pn: int) -> bytes:
    """The first pn_off bytes of raw and the low pn_len bytes of pn, big-endian."""
    pn_len = pn_len_of(raw[0])
    return bytes(raw[:pn_off]) + (pn & ((1 << (8 * pn_len)) - 1)).to_bytes(pn_len, "big")


def apply_hp(hp: bytes, pkt: bytes, pn_off: int) -> bytes:
    """Header protection over header || ciphertext || tag (its first byte unprotected)."""
    pkt = bytearray(pkt)
    pn_len = pn_len_of(pkt[0])
    mask = hp_mask(hp, bytes(pkt[pn_off + 4:pn_off + 4 + SAMPLE_LEN]))
    pkt[0] ^= mask[0] & first_byte_bits(pkt[0])
    for j in range(pn_len):
        pkt[pn_off + j] ^= mask[1 + j]
    return bytes(pkt)


def protect(key: bytes, iv: bytes, hp: bytes, pn: int, raw: bytes, pn_off: int):
    """raw = header || payload (the packet number field's bytes are ignored) -> the protected
    packet, len(raw) + 16 bytes; None where there is no full sample (the sender has to pad)."""
    if len(raw) <= pn_off:
        return None
    pn_len = pn_len_of(raw[0])
    hdr_len = pn_off + pn_len
    if len(raw) < hdr_len or pn_len + len(raw) - hdr_len < 4:
        return None
    header = header_of(raw, pn_off, pn)
    body = R.seal(key, nonce_of(iv, pn), bytes(raw[hdr_len:]), header)
    return apply_hp(hp, header + body, pn_off)


def decode_pn(expected_pn: int, truncated: int, pn_len: int) -> int:
    """RFC 9000 appendix A.3, DecodePacketNumber with largest_pn = expected_pn - 1."""
    pn_win = 1 << (8 * pn_len)
    pn_hwin, pn_mask = pn_win // 2, pn_win - 1
    candidate = (expected_pn & ~pn_mask) | (truncated & pn_mask)
    if candidate <= expected_pn - pn_hwin and candidate < (1 << 62) - pn_win:
        return candidate + pn_win
    if candidate > expected_pn + pn_hwin and candidate >= pn_win:
        return candidate - pn_win
    return candidate


def unprotect(keys, ivs, hp: bytes, expected_pn: int, pkt: bytes, pn_off: int):
    """(rc, header || plaintext, pn): rc 2 and nothing for a packet shorter than pn_off + 20;
    else rc 0 or 1 (wrong tag) with the decryption, which always runs.  keys / ivs: one key
    and IV, or a pair of each, of which a short-header packet takes the one its key phase
    bit names and a long-header packet the first."""
    if len(pkt) < pn_off + 4 + SAMPLE_LEN:
        return 2, b"", 0
    mask = hp_mask(hp, bytes(pkt[pn_off + 4:pn_off + 4 + SAMPLE_LEN]))
    b0 = pkt[0] ^ (mask[0] & first_byte_bits(pkt[0]))
    pn_len = pn_len_of(b0)
    hdr_len = pn_off + pn_len
    trunc = int.from_bytes(bytes(a ^ b for a, b in zip(pkt[pn_off:hdr_len], mask[1:])), "big")
    pn = decode_pn(expected_pn, trunc, pn_len)
    header = bytes([b0]) + bytes(pkt[1:pn_off]) + trunc.to_bytes(pn_len, "big")
    phase = 0 if b0 & 0x80 else (b0 >> 2) & 1
    key, iv = (keys, ivs) if isinstance(keys, (bytes, bytearray)) else (keys[phase], ivs[phase])
    rc, pt = R.open(key, nonce_of(iv, pn), bytes(pkt[hdr_len:]), header)
    return rc, header + pt, pn


def golden() -> dict:
    return json.loads(GOLDEN.read_text())
