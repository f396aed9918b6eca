#!/usr/bin/env python3
"""Writes tests/golden/dtls13_records.json from OpenSSL alone.

DTLS 1.3 records under TLS_CHACHA20_POLY1305_SHA256 as RFC 9147 section 4 defines them: the
unified header 001CSLEE || cid || the sequence number's low 8 or 16 bits || optionally
be16(length of the encrypted record); the nonce the 12-byte IV XOR the left-padded 64-bit
sequence number; the plaintext content || type || zeros; the additional data that header;
the AEAD RFC 8439; and the record number mask (section 4.2.3) the first bytes of ChaCha20
under sn_key with the first 16 bytes of the encrypted record as counter and nonce.  RFC 9147
has no record vectors and OpenSSL speaks no DTLS 1.3, so header, nonce and inner plaintext
are built here by their definitions; every record is sealed by OpenSSL's EVP
"ChaCha20-Poly1305" (tests/rfc8439_ref.openssl()) and masked with OpenSSL's EVP "ChaCha20",
whose 16-byte IV is le32(counter) || nonce.  Nothing of the project's own arithmetic enters
the file.  The content of a case is SHAKE-256("dtls13 content <n>") (rfc8439_ref.data) and
the connection ID SHAKE-256("dtls13 cid <cid_len>"), so only the protected header, the mask,
the tag and a SHA-256 of the ciphertext are stored.

Usage: python tests/golden/make_dtls13_records.py
"""
from __future__ import annotations

import ctypes as C
import hashlib
import json
import struct
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
import rfc8439_ref as R  # noqa: E402

OUT = HERE / "dtls13_records.json"
KEY = hashlib.sha256(b"dtls13 golden key").digest()
IV = hashlib.sha256(b"dtls13 golden iv").digest()[:12]
SN = hashlib.sha256(b"dtls13 golden sn").digest()
LENGTHS = (0, 1, 14, 15, 16, 63, 64, 1431)
CID_LENS = (0, 1, 11, 12, 250)
SEQS = (0, 2**16 - 1, 2**48 - 1)
TYPES = (23, 22, 21, 26)
# (content length, pad_to): made bytes inside a chunk, on a chunk edge, over whole chunks, and the cap
PADDED = ((0, 16), (15, 16), (16, 16), (62, 64), (63, 64), (64, 64), (100, 256), (1431, 256), (16383, 256), (16384, 256),
          (10000, 10000))


def mask_of(ossl, sn_key: bytes, sample: bytes) -> bytes:
    """EVP "ChaCha20" over two zero bytes with the sample as IV."""
    L = ossl.L
    cipher = L.EVP_CIPHER_fetch(None, b"ChaCha20", None)
    assert cipher
    ctx = L.EVP_CIPHER_CTX_new()
    try:
        assert L.EVP_EncryptInit_ex(ctx, cipher, None, sn_key, sample) == 1
        out, ol = C.create_string_buffer(2), C.c_int(0)
        assert L.EVP_EncryptUpdate(ctx, out, C.byref(ol), bytes(2), 2) == 1 and ol.value == 2
        return out.raw
    finally:
        L.EVP_CIPHER_CTX_free(ctx)


def main() -> int:
    ossl = R.openssl()
    if ossl is None:
        print("libcrypto with ChaCha20-Poly1305 is needed to write the fixture", file=sys.stderr)
        return 1
    cases = []

    def add(n, seq16, length, cid_len, seq, epoch, ctype, pad_to):
        inner = n + 1
        if pad_to > 1 and inner < 2**14 + 1:
            inner = min((inner + pad_to - 1) // pad_to * pad_to, 2**14 + 1)
        pt = R.data(n, b"dtls13 content %d" % n) + bytes([ctype]) + bytes(inner - n - 1)
        cid = R.data(cid_len, b"dtls13 cid %d" % cid_len)
        sn = 2 if seq16 else 1
        b0 = 0x20 | (0x10 if cid_len else 0) | (0x08 if seq16 else 0) | (0x04 if length else 0) | (epoch % 4)
        header = bytes([b0]) + cid + (seq % 256**sn).to_bytes(sn, "big") + (struct.pack(">H", inner + 16) if length else b"")
        nonce = bytes(a ^ b for a, b in zip(IV, seq.to_bytes(12, "big")))
        sealed = ossl.seal(KEY, nonce, pt, header)
        sample = sealed[:16]
        mask = mask_of(ossl, SN, sample)
        prot = bytearray(header)
        for j in range(sn):
            prot[1 + cid_len + j] ^= mask[j]
        cases.append({"n": n, "seq16": seq16, "length": length, "cid_len": cid_len, "seq": seq, "epoch": epoch, "type": ctype,
                      "pad_to": pad_to, "inner": inner, "nonce": nonce.hex(), "mask": mask.hex(),
                      "protected_header": (bytes(prot[:1]) + bytes(prot[1 + cid_len:])).hex(),
                      "ct_sha256": hashlib.sha256(sealed[:-16]).hexdigest(), "tag": sealed[-16:].hex()})

    k = 0
    for n in LENGTHS:
        for seq16 in (False, True):
            for length in (False, True):
                for cid_len in CID_LENS:
                    for seq in SEQS:
                        add(n, seq16, length, cid_len, seq, k % 4, TYPES[k % 4], 0)
                        k += 1
    for i, (n, pad_to) in enumerate(PADDED):
        add(n, bool(i & 1), bool(i & 2), CID_LENS[i % 5], SEQS[i % 3], i % 4, TYPES[i % 4], pad_to)
    doc = {"source": "OpenSSL EVP ChaCha20-Poly1305 and ChaCha20 (" + ossl.version + ")", "key": KEY.hex(), "iv": IV.hex(),
           "sn_key": SN.hex(), "content": "SHAKE-256('dtls13 content <n>'), then the type byte and zeros up to `inner`",
           "cid": "SHAKE-256('dtls13 cid <cid_len>')",
           "protected_header": "the first byte and the bytes behind the connection ID (masked sequence number, length)",
           "cases": cases}
    OUT.write_text(json.dumps(doc, separators=(",", ":")) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases")
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
