#!/usr/bin/env python3
"""Writes tests/golden/wg_packets.json from OpenSSL alone.

WireGuard transport data messages as the whitepaper's section 5.4.6 defines them: the
header le32(4) || le32(receiver) || le64(counter), the nonce four zero bytes and
le64(counter), the plaintext the inner packet with zeros up to a multiple of 16 (at most
max(len, pad_cap) where there is a pad_cap), no additional data, the AEAD RFC 8439.  Nonce,
header and padding are built here by their definitions; every message is sealed by
OpenSSL's EVP "ChaCha20-Poly1305" (tests/rfc8439_ref.openssl()).  Nothing of the project's
own arithmetic enters the file.  The inner packet of a case is SHAKE-256("wg inner <n>")
(rfc8439_ref.data), so only the header, the padded length, the tag and a SHA-256 of the
ciphertext are stored.

Usage: python tests/golden/make_wg_packets.py
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

OUT = HERE / "wg_packets.json"
KEY = hashlib.sha256(b"wg golden key").digest()
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 1420, 1500)
COUNTERS = (0, 2**32 - 1, 2**32, 2**64 - 2**13 - 2)
PAD_CAPS = (0, 1420, 1500)


def main() -> int:
    ossl = R.openssl()
    if ossl is None:
        print("libcrypto with ChaCha20-Poly1305 is needed to write the fixture", file=sys.stderr)
        return 1
    cases = []
    for n in LENGTHS:
        for k, counter in enumerate(COUNTERS):
            for cap in PAD_CAPS:
                padded = (n + 15) // 16 * 16
                if cap:
                    padded = min(padded, max(n, cap))
                receiver = int.from_bytes(hashlib.sha256(b"wg receiver %d %d" % (n, k)).digest()[:4], "little")
                header = struct.pack("<I", 4) + struct.pack("<I", receiver) + struct.pack("<Q", counter)
                nonce = bytes(4) + struct.pack("<Q", counter)
                sealed = ossl.seal(KEY, nonce, R.data(n, b"wg inner %d" % n) + bytes(padded - n), b"")
                cases.append({"n": n, "pad_cap": cap, "receiver": receiver, "counter": counter, "padded": padded,
                              "header": header.hex(), "nonce": nonce.hex(),
                              "ct_sha256": hashlib.sha256(sealed[:-16]).hexdigest(), "tag": sealed[-16:].hex()})
    doc = {"source": "OpenSSL EVP ChaCha20-Poly1305 (" + ossl.version + ")", "key": KEY.hex(),
           "inner": "SHAKE-256('wg inner <n>'), zeros up to `padded`", "cases": cases}
    OUT.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
