#!/usr/bin/env python3
"""Writes tests/golden/tls13_keys.json from OpenSSL alone.

HKDF-Expand-Label (RFC 8446 section 7.1) as OpenSSL's TLS13-KDF computes it,
through the command line:

    openssl kdf -keylen L -kdfopt digest:SHA256 -kdfopt mode:EXPAND_ONLY \\
        -kdfopt hexkey:<secret> -kdfopt hexprefix:<"tls13 "> -kdfopt hexlabel:<label> TLS13-KDF

for the three labels of the traffic keys -- "key" (32 bytes), "iv" (12) and
"traffic upd" (32), all with an empty context -- over a few secrets, and a
chain of three updates with the keys of every generation.  Nothing of the
project's own arithmetic, and nothing of tests/tls13_keys_ref.py, enters the
file.  Needs OpenSSL 3.0 or later.

Usage: python tests/golden/make_tls13_keys.py
"""
from __future__ import annotations

import hashlib
import json
import subprocess
import sys
from pathlib import Path

OUT = Path(__file__).resolve().parent / "tls13_keys.json"
LABELS = (("key", 32), ("iv", 12), ("traffic upd", 32))
SECRETS = [hashlib.shake_256(b"tls13 golden secret %d" % i).digest(32) for i in range(3)] + [bytes(32), b"\xff" * 32]
CHAIN = 3


def tls13_kdf(secret: bytes, label: str, length: int) -> bytes:
    cmd = ["openssl", "kdf", "-keylen", str(length), "-kdfopt", "digest:SHA256", "-kdfopt", "mode:EXPAND_ONLY",
           "-kdfopt", "hexkey:" + secret.hex(), "-kdfopt", "hexprefix:" + b"tls13 ".hex(),
           "-kdfopt", "hexlabel:" + label.encode().hex(), "TLS13-KDF"]
    p = subprocess.run(cmd, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError("openssl kdf failed: " + p.stderr.strip())
    out = bytes.fromhex(p.stdout.strip().replace(":", ""))
    assert len(out) == length
    return out


def main() -> int:
    try:
        version = subprocess.run(["openssl", "version"], capture_output=True, text=True, check=True).stdout.strip()
    except (OSError, subprocess.CalledProcessError):
        print("the openssl command line tool (3.0 or later) is needed to write the fixture", file=sys.stderr)
        return 1
    cases = [{"secret": s.hex(), **{label: tls13_kdf(s, label, n).hex() for label, n in LABELS}} for s in SECRETS]
    chain, s = [], SECRETS[0]
    for _ in range(CHAIN + 1):  # generation 0 .. CHAIN
        chain.append({"secret": s.hex(), "key": tls13_kdf(s, "key", 32).hex(), "iv": tls13_kdf(s, "iv", 12).hex()})
        s = tls13_kdf(s, "traffic upd", 32)
    doc = {"source": "openssl kdf TLS13-KDF, mode EXPAND_ONLY, digest SHA256, prefix 'tls13 ' (" + version + ")",
           "labels": {label: n for label, n in LABELS}, "cases": cases, "chain": chain}
    OUT.write_text(json.dumps(doc, indent=1) + "\n")
    print(OUT, OUT.stat().st_size, "bytes,", len(cases), "cases, chain of", CHAIN)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
