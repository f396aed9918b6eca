#!/usr/bin/env python3
"""Generate tests/golden/rfc8439_vectors.json from OpenSSL 3.

Every vector is the output of libcrypto's own AEAD (EVP_CIPHER_fetch
"ChaCha20-Poly1305", IV length 12); nothing here is computed by the project's
code or by the tests' restatement (tests/rfc8439_ref.py), which only supplies
the inputs: the shapes of the GPU tests and their bytes (SHAKE-256 of the
shape's name).

* ``small``: full vectors, n and adlen over {0, 1, 15, 16, 17, 63, 64, 65}.
* ``shapes``: every shape of tests/test_gpu_msg_rfc8439.py and every message of
  tests/test_gpu_msg_batch_rfc8439.py as tag and SHA-256 of the ciphertext; the
  inputs follow from (n, adlen) or the message's index.

The file depends on the inputs alone: running this again rewrites it byte for
byte.

Usage:  python tests/golden/make_rfc8439_golden.py
"""
from __future__ import annotations

import hashlib
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))

import rfc8439_ref as ref  # noqa: E402


def main() -> None:
    ossl = ref.OpenSSL()
    small = []
    for n in ref.SMALL:
        for adlen in ref.SMALL:
            key, nonce, pt, ad = ref.single_message(n, adlen)
            small.append({"n": n, "adlen": adlen, "key": key.hex(), "nonce": nonce.hex(), "pt": pt.hex(),
                          "ad": ad.hex(), "ct_tag": ossl.seal(key, nonce, pt, ad).hex()})

    def digest(out: bytes) -> dict:
        return {"tag": out[-16:].hex(), "ct_sha256": hashlib.sha256(out[:-16]).hexdigest()}

    single = []
    for n, adlen in ref.single_shapes() + [((1 << 20) + 7, 13)]:
        key, nonce, pt, ad = ref.single_message(n, adlen)
        single.append({"n": n, "adlen": adlen, **digest(ossl.seal(key, nonce, pt, ad))})
    batch = []
    for i, (adlen, n) in enumerate(ref.batch_shapes()):
        kidx, nonce, pt, ad = ref.batch_message(i, adlen, n)
        batch.append({"index": i, "n": n, "adlen": adlen, "key_index": kidx, "nonce": nonce.hex(),
                      **digest(ossl.seal(ref.KEYS[32 * kidx:32 * kidx + 32], nonce, pt, ad))})
    doc = {
        "construction": "RFC 8439 AEAD_CHACHA20_POLY1305 (96-bit nonce, padded MAC stream)",
        "generator": "tests/golden/make_rfc8439_golden.py (OpenSSL EVP_CIPHER_fetch \"ChaCha20-Poly1305\", IV length 12)",
        "openssl": ossl.version,
        "data_rule": "tests/rfc8439_ref.py: single_message(n, adlen) and batch_message(index, adlen, n), SHAKE-256",
        "key": ref.KEY.hex(), "nonce": ref.NONCE.hex(), "batch_keys": ref.KEYS.hex(),
        "small": small, "shapes": {"single": single, "batch": batch},
    }
    ref.GOLDEN.write_text(json.dumps(doc, indent=1) + "\n")
    print(f"wrote {len(small)} full vectors, {len(single)} + {len(batch)} digests ({ossl.version})")


if __name__ == "__main__":
    main()
