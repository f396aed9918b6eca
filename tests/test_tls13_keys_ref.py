"""The HKDF / traffic-key reference (tests/tls13_keys_ref.py) against OpenSSL's
TLS13-KDF (tests/golden/tls13_keys.json, written by tests/golden/make_tls13_keys.py),
and against RFC 5869's own test vectors for Extract and the general Expand.  CPU only."""
from __future__ import annotations

import json
from pathlib import Path

import pytest

import tls13_keys_ref as R

DOC = json.loads((Path(__file__).resolve().parent / "golden" / "tls13_keys.json").read_text())


def test_fixture_covers_the_cases():
    assert "TLS13-KDF" in DOC["source"] and "OpenSSL" in DOC["source"]
    assert DOC["labels"] == {"key": 32, "iv": 12, "traffic upd": 32}
    secrets = [bytes.fromhex(c["secret"]) for c in DOC["cases"]]
    assert bytes(32) in secrets and b"\xff" * 32 in secrets and len(set(secrets)) == len(secrets) >= 5
    assert len(DOC["chain"]) == 4 and DOC["chain"][0]["secret"] == DOC["cases"][0]["secret"]


@pytest.mark.parametrize("i", range(len(DOC["cases"])))
def test_labels_against_openssl_fixture(i):
    c = DOC["cases"][i]
    s = bytes.fromhex(c["secret"])
    for label, n in DOC["labels"].items():
        assert R.expand_label(s, label.encode(), b"", n).hex() == c[label], label
    assert R.traffic_keys(s) == (bytes.fromhex(c["key"]), bytes.fromhex(c["iv"]))
    assert R.next_secret(s).hex() == c["traffic upd"]


def test_update_chain_against_openssl_fixture():
    s = bytes.fromhex(DOC["chain"][0]["secret"])
    for g, c in enumerate(DOC["chain"]):
        assert R.generation(s, g).hex() == c["secret"], g
        assert R.traffic_keys(R.generation(s, g)) == (bytes.fromhex(c["key"]), bytes.fromhex(c["iv"])), g


def test_hkdf_label_bytes():
    assert R.hkdf_label(32, b"key", b"") == bytes.fromhex("0020" "09" "746c733133206b6579" "00")
    assert R.hkdf_label(12, b"iv", b"") == bytes.fromhex("000c" "08" "746c733133206976" "00")
    assert R.hkdf_label(32, b"traffic upd", b"") == b"\x00\x20\x11tls13 traffic upd\x00"
    assert R.hkdf_label(300, b"", b"\x01\x02") == b"\x01\x2c\x06tls13 \x02\x01\x02"


def test_rfc5869_vectors():
    """RFC 5869 appendix A.1 and A.3 (SHA-256): Extract with and without a salt, the general Expand."""
    ikm = bytes([0x0B] * 22)
    prk = R.extract(bytes(range(13)), ikm)
    assert prk.hex() == "077709362c2e32df0ddc3f0dc47bba6390b6c73bb50f9c3122ec844ad7c2b3e5"
    assert R.expand(prk, bytes(range(0xF0, 0xFA)), 42).hex() == (
        "3cb25f25faacd57a90434f64d0362f2a2d2d0a90cf1a5a4c5db02d56ecc4c5bf34007208d5b887185865")
    prk = R.extract(b"", ikm)
    assert prk.hex() == "19ef24a32c717b167f33a91d6f648bdf96596776afdb6377ac434c1c293ccb04"
    assert R.expand(prk, b"", 42).hex() == (
        "8da4e775a563c18f715f802a063c5a31b8a11f5c5ee1879ec3454e5f3c738d2d9d201395faa4b61a96c8")
    assert R.expand(prk, b"x", 0) == b""


def test_test_secrets_have_the_edge_rows():
    rows = R.secrets(5)
    assert rows[0] == bytes(32) and rows[1] == b"\xff" * 32 and all(r[0] & 0x80 for r in rows[2:])
    assert len(set(rows)) == 5 and R.secrets(1) == [bytes(32)]
