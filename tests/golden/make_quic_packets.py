#!/usr/bin/env python3
"""Writes tests/golden/quic_packets.json from OpenSSL alone.

QUIC packets under AEAD_CHACHA20_POLY1305 as RFC 9001 section 5.3 - 5.4 defines them: the
nonce is the 12-byte IV XOR the left-padded packet number, the additional data the packet's
header with the packet number's low pn_len bytes, the AEAD RFC 8439, and the header
protection mask the first five bytes of ChaCha20 under the header protection key with the
16-byte sample as counter and nonce.  Nonce and header are built here by their definitions;
every packet is sealed by OpenSSL's EVP "ChaCha20-Poly1305" (tests/rfc8439_ref.openssl())
and masked with OpenSSL's EVP "ChaCha20", whose 16-byte IV is le32(counter) || nonce:
section 5.4.4's definition word for word.  Nothing of the project's own arithmetic enters
the file.  The payload of a case is SHAKE-256("quic payload <n>") (rfc8439_ref.data) and
the header's other bytes SHAKE-256("quic header <pn_off>"), so only the protected header,
the tag and a SHA-256 of the ciphertext are stored.

Usage: python tests/golden/make_quic_packets.py
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import rfc8439_ref as R  # noqa: E402

OUT = HERE / "quic_packets.json"
KEY = hashlib.sha256(b"quic golden key").digest()
IV = hashlib.sha256(b"quic golden iv").digest()[:12]
HP = hashlib.sha256(b"quic golden hp").digest()
# (first byte, pn_off, payload length, packet number)
CASES = [(0x40 | (pn_len - 1) | phase << 2, pn_off, n, pn)
         for pn_len, n in ((1, 3), (2, 2), (3, 1), (4, 0), (1, 16), (2, 63), (3, 64), (4, 1431))
         for pn_off, phase, pn in ((1, 0, 0), (9, 1, 2**32 - 1), (21, 0, 2**62 - 1))]
CASES += [(0xC0 | (pn_len - 1), 251, 100, 2**32) for pn_len in (1, 4)]  # long header: a 4-bit mask


def mask_of(ossl, hp: bytes, sample: bytes) -> bytes:
    """EVP "ChaCha20" over five zero bytes with the sample as IV."""
    L = ossl.L
    cipher = L.EVP_CIPHER_fetch(None, b"ChaCha20", None)
    assert cipher
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        assert L.EVP_EncryptInit_ex(ctx, cipher, None, hp, sample) == 1
        out, ol = C.create_string_buffer(5), C.c_int(0)
        assert L.EVP_EncryptUpdate(ctx, out, C.byref(ol), bytes(5), 5) == 1 and ol.value == 5
        return out.raw
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def main() -> int:
    ossl = R.openssl()
    if ossl is None:
        print("libcrypto with ChaCha20-Poly1305 is needed to write the fixture", file=sys.stderr)
        return 1
    cases = []
    for b0, pn_off, n, pn in CASES:
        pn_len = (b0 & 3) + 1
        header = bytes([b0]) + R.data(pn_off - 1, b"quic header %d" % pn_off) + (pn % 256**pn_len).to_bytes(pn_len, "big")
        nonce = bytes(a ^ b for a, b in zip(IV, pn.to_bytes(12, "big")))
        sealed = ossl.seal(KEY, nonce, R.data(n, b"quic payload %d" % n), header)
        pkt = bytearray(header + sealed)
        sample = bytes(pkt[pn_off + 4:pn_off + 20])
        mask = mask_of(ossl, HP, sample)
        pkt[0] ^= mask[0] & (0x0F if b0 & 0x80 else 0x1F)
        for j in range(pn_len):
            pkt[pn_off + j] ^= mask[1 + j]
        cases.append({"first": b0, "pn_off": pn_off, "n": n, "pn": pn, "nonce": nonce.hex(), "sample": sample.hex(),
                      "mask": mask.hex(), "protected_header": bytes(pkt[:len(header)]).hex(),
                      "ct_sha256": hashlib.sha256(sealed[:-16]).hexdigest(), "tag": sealed[-16:].hex()})
    doc = {"source": "OpenSSL EVP ChaCha20-Poly1305 and ChaCha20 (" + ossl.version + ")", "key": KEY.hex(),
           "iv": IV.hex(), "hp": HP.hex(), "payload": "SHAKE-256('quic payload <n>')",
           "header": "first || SHAKE-256('quic header <pn_off>')[:pn_off - 1] || pn bytes", "cases": cases}
    OUT.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
