#!/usr/bin/env python3
"""Writes tests/golden/esp_packets.json from OpenSSL alone.

IPsec ESP packets with ChaCha20-Poly1305 as RFC 7634 over RFC 4303 defines them: the header
be32(spi) || be32(seq_lo) || be64(iv), the nonce salt || be64(iv), the plaintext the payload,
the padding bytes 1 .. pad, u8(pad) and u8(next_header) with payload, padding and trailer
ending on a multiple of `align`, the additional data be32(spi) || be32(seq_lo) or, with
extended sequence numbers, be32(spi) || be32(seq_hi) || be32(seq_lo), the AEAD RFC 8439.
Header, nonce, additional data and trailer are built here by their definitions; every
packet is sealed by OpenSSL's EVP "ChaCha20-Poly1305" (tests/rfc8439_ref.openssl()).
Nothing of the project's own arithmetic enters the file.  The payload of a case is
SHAKE-256("esp payload <n>") (rfc8439_ref.data), so only the header, the nonce, the
additional data, the padded length, the ICV and a SHA-256 of the ciphertext are stored.
Without ESN the sequence number is taken mod 2^32, also where it stands in for the IV.

The last case has the inputs of RFC 7634 appendix A as far as they are structural (key
80..9f, salt a0 a1 a2 a3, SPI 01020304, sequence number 5, IV 10..17, 84 bytes of payload,
next header 4: pad 2, trailer 01 02 02 04); its payload is given in full, its expected
bytes are OpenSSL's like all others.

Usage: python tests/golden/make_esp_packets.py
"""
from __future__ import annotations

import hashlib
import json
import struct
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import rfc8439_ref as R  # noqa: E402

OUT = HERE / "esp_packets.json"
KEY = hashlib.sha256(b"esp golden key").digest()
SALT = hashlib.sha256(b"esp golden salt").digest()[:4]
LENGTHS = (0, 1, 2, 61, 62, 63, 64, 1400, 1438)
ALIGNS = (4, 16, 256)
SEQS = (0, 2**32 - 1, 2**32, 2**64 - 1)
NEXT_HEADERS = (4, 41, 59, 255)


def packet(ossl, key, salt, spi, seq, iv, payload, next_header, align, esn):
    """(header, nonce, ad, padded, sealed) by the definitions above."""
    if not esn:
        seq %= 2**32
    if iv is None:
        iv = seq
    pad = (align - (len(payload) + 2) % align) % align
    pt = payload + bytes(range(1, pad + 1)) + bytes([pad, next_header])
    lo, hi = seq % 2**32, seq >> 32
    header = struct.pack(">I", spi) + struct.pack(">I", lo) + struct.pack(">Q", iv)
    nonce = salt + struct.pack(">Q", iv)
    ad = struct.pack(">I", spi) + (struct.pack(">I", hi) if esn else b"") + struct.pack(">I", lo)
    return header, nonce, ad, len(pt), ossl.seal(key, nonce, pt, ad)


def main() -> int:
    ossl = R.openssl()
    if ossl is None:
        print("libcrypto with ChaCha20-Poly1305 is needed to write the fixture", file=sys.stderr)
        return 1
    cases = []

    def add(key, salt, spi, seq, iv, payload, nh, align, esn, more=None):
        header, nonce, ad, padded, sealed = packet(ossl, key, salt, spi, seq, iv, payload, nh, align, esn)
        cases.append({"n": len(payload), "align": align, "esn": esn, "spi": spi, "seq": seq, "iv": iv, "next_header": nh,
                      "padded": padded, "header": header.hex(), "nonce": nonce.hex(), "ad": ad.hex(),
                      "ct_sha256": hashlib.sha256(sealed[:-16]).hexdigest(), "icv": sealed[-16:].hex(), **(more or {})})

    for n in LENGTHS:
        for align in ALIGNS:
            for esn in (False, True):
                for k, seq in enumerate(SEQS):
                    for given in (False, True):
                        what = b"esp %d %d %d %d" % (n, align, esn, k)
                        spi = int.from_bytes(hashlib.sha256(b"spi " + what).digest()[:4], "big")
                        iv = int.from_bytes(hashlib.sha256(b"iv " + what).digest()[:8], "big") if given else None
                        add(KEY, SALT, spi, seq, iv, R.data(n, b"esp payload %d" % n), NEXT_HEADERS[k], align, esn)
    a_payload = R.data(84, b"esp rfc7634 appendix a payload")
    add(bytes(range(0x80, 0xA0)), bytes.fromhex("a0a1a2a3"), 0x01020304, 5, 0x1011121314151617, a_payload, 4, 4, False,
        {"key": bytes(range(0x80, 0xA0)).hex(), "salt": "a0a1a2a3", "payload": a_payload.hex()})
    doc = {"source": "OpenSSL EVP ChaCha20-Poly1305 (" + ossl.version + ")", "key": KEY.hex(), "salt": SALT.hex(),
           "payload": "SHAKE-256('esp payload <n>'), then 01 02 .. pad, pad, next_header up to `padded`", "cases": cases}
    OUT.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
