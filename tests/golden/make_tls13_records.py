#!/usr/bin/env python3
"""Writes tests/golden/tls13_records.json from OpenSSL alone.

TLS 1.3 records under TLS_CHACHA20_POLY1305_SHA256 as RFC 8446 section 5.2 - 5.4
defines them: the nonce is the 12-byte write IV XOR the left-padded sequence
number, the additional data the record header 17 03 03 be16(fragment length),
the plaintext TLSInnerPlaintext = content || type || zeros, the AEAD RFC 8439.
Nonce, header and inner plaintext are built here by their definitions and every
record is sealed by OpenSSL's EVP "ChaCha20-Poly1305"
(tests/rfc8439_ref.openssl()); nothing of the project's own arithmetic enters
the file.  The content of a case is SHAKE-256("tls13 content <n>")
(rfc8439_ref.data), so only the tag and a SHA-256 of the ciphertext are stored.

Usage: python tests/golden/make_tls13_records.py
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

OUT = HERE / "tls13_records.json"
KEY = hashlib.sha256(b"tls13 golden key").digest()
IVS = [hashlib.sha256(b"tls13 golden iv").digest()[:12], b"\xff" * 12]
LENGTHS = (0, 1, 15, 16, 100, 16384)
SEQS = (0, 2**32 - 1, 2**64 - 1)
CTYPE = 23   # application_data
PADDED = 100  # the content length that is also sealed with PAD zeros of padding
PAD = 7


def main() -> int:
    ossl = R.openssl()
    if ossl is None:
        print("libcrypto with ChaCha20-Poly1305 is needed to write the fixture", file=sys.stderr)
        return 1
    cases = []
    for iv_i, iv in enumerate(IVS):
        for seq in SEQS:
            for n, pad in [(n, 0) for n in LENGTHS] + [(PADDED, PAD)]:
                nonce = bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", seq)))
                inner = R.data(n, b"tls13 content %d" % n) + bytes([CTYPE]) + bytes(pad)
                ad = struct.pack(">BBBH", 23, 3, 3, len(inner) + 16)
                sealed = ossl.seal(KEY, nonce, inner, ad)
                cases.append({"iv": iv_i, "seq": seq, "n": n, "pad": pad, "nonce": nonce.hex(), "ad": ad.hex(),
                              "ct_sha256": hashlib.sha256(sealed[:-16]).hexdigest(), "tag": sealed[-16:].hex()})
    doc = {"source": "OpenSSL EVP ChaCha20-Poly1305 (" + ossl.version + ")", "key": KEY.hex(),
           "ivs": [iv.hex() for iv in IVS], "type": CTYPE, "content": "SHAKE-256('tls13 content <n>')", "cases": cases}
    OUT.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
