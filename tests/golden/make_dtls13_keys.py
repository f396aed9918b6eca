#!/usr/bin/env python3
"""Writes tests/golden/dtls13_keys.json from hashlib's HMAC-SHA-256 alone.

HKDF-Expand-Label (RFC 8446 section 7.1) with DTLS 1.3's label prefix "dtls13" (RFC 9147
section 5.9; no trailing space), built here by its definition:

    HkdfLabel = be16(length) || u8(6 + |label|) || "dtls13" || label || u8(0)
    T(1)      = HMAC-SHA-256(secret, HkdfLabel || 01), cut to `length` (at most 32 here)

for the labels of the record protection keys -- "key" (32 bytes), "iv" (12), "sn" (32) and
"traffic upd" (32), all with an empty context -- over a few secrets, and a chain of three
updates with the keys of every generation.  Nothing of the project's own arithmetic, and
nothing of tests/dtls13_ref.py, enters the file.

Usage: python tests/golden/make_dtls13_keys.py
"""
from __future__ import annotations

import hashlib
import hmac
import json
from pathlib import Path

OUT = Path(__file__).resolve().parent / "dtls13_keys.json"
LABELS = (("key", 32), ("iv", 12), ("sn", 32), ("traffic upd", 32))
SECRETS = [hashlib.shake_256(b"dtls13 golden secret %d" % i).digest(32) for i in range(3)] + [bytes(32), b"\xff" * 32]
CHAIN = 3


def expand_label(secret: bytes, label: str, length: int) -> bytes:
    assert length <= 32
    full = b"dtls13" + label.encode()
    info = length.to_bytes(2, "big") + bytes([len(full)]) + full + b"\x00"
    return hmac.new(secret, info + b"\x01", hashlib.sha256).digest()[:length]


def main() -> int:
    cases = [{"secret": s.hex(), **{label: expand_label(s, label, n).hex() for label, n in LABELS}} for s in SECRETS]
    chain, s = [], SECRETS[0]
    for _ in range(CHAIN + 1):  # generation 0 .. CHAIN
        chain.append({"secret": s.hex(), **{label: expand_label(s, label, n).hex() for label, n in LABELS[:3]}})
        s = expand_label(s, "traffic upd", 32)
    doc = {"source": "hashlib HMAC-SHA-256, HkdfLabel with the prefix 'dtls13'", "labels": {label: n for label, n in LABELS},
           "cases": cases, "chain": chain}
    OUT.write_text(json.dumps(doc, indent=1) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases, chain of", CHAIN)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
