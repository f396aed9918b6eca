#!/usr/bin/env python3
"""Writes tests/golden/rfc7905_records.json from OpenSSL alone.

TLS 1.2 ChaCha20-Poly1305 records as RFC 7905 section 2 defines them: the nonce
is the 12-byte write IV XOR the left-padded sequence number, the additional data
the 13 bytes seq || type || version || length, the AEAD RFC 8439.  The nonce and
the AD are built here by their definitions and every record is sealed by
OpenSSL's EVP "ChaCha20-Poly1305" (tests/rfc8439_ref.openssl()); nothing of the
project's own arithmetic enters the file.  The plaintext of a case is
SHAKE-256("rfc7905 pt <n>") (rfc8439_ref.data), so only the tag and a SHA-256 of
the ciphertext are stored.

Usage: python tests/golden/make_rfc7905_records.py
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

OUT = HERE / "rfc7905_records.json"
KEY = hashlib.sha256(b"rfc7905 golden key").digest()
IVS = [hashlib.sha256(b"rfc7905 golden iv").digest()[:12], b"\xff" * 12]
LENGTHS = (0, 1, 16, 100, 16384)
SEQS = (0, 2**32 - 1, 2**64 - 1)
HEADER = (23, 3, 3)  # application_data, TLS 1.2


def main() -> int:
    ossl = R.openssl()
    if ossl is None:
        print("libcrypto with ChaCha20-Poly1305 is needed to write the fixture", file=sys.stderr)
        return 1
    cases = []
    for iv_i, iv in enumerate(IVS):
        for seq in SEQS:
            for n in LENGTHS:
                nonce = bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", seq)))
                ad = struct.pack(">QBBBH", seq, *HEADER, n)
                sealed = ossl.seal(KEY, nonce, R.data(n, b"rfc7905 pt %d" % n), ad)
                cases.append({"iv": iv_i, "seq": seq, "n": n, "nonce": nonce.hex(), "ad": ad.hex(),
                              "ct_sha256": hashlib.sha256(sealed[:-16]).hexdigest(), "tag": sealed[-16:].hex()})
    doc = {"source": "OpenSSL EVP ChaCha20-Poly1305 (" + ossl.version + ")", "key": KEY.hex(),
           "ivs": [iv.hex() for iv in IVS], "header": list(HEADER), "pt": "SHAKE-256('rfc7905 pt <n>')", "cases": cases}
    OUT.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
