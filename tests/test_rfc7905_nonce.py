"""The RFC 7905 nonce rule (write IV XOR sequence number) and the 13-byte TLS 1.2
additional data as the RFC batch tests state them in Python
(tests/rfc_batch_support.py), pinned to records OpenSSL sealed
(tests/golden/rfc7905_records.json, written by tests/golden/make_rfc7905_records.py).
CPU only."""
from __future__ import annotations

import hashlib
import json
import struct
from pathlib import Path

import pytest

import rfc8439_ref as R
import rfc_batch_support as S

DOC = json.loads((Path(__file__).resolve().parent / "golden" / "rfc7905_records.json").read_text())
KEY = bytes.fromhex(DOC["key"])
IVS = [bytes.fromhex(x) for x in DOC["ivs"]]


def test_fixture_covers_the_edges():
    cases = DOC["cases"]
    assert {c["n"] for c in cases} >= {0, 1, 16, 100, 16384}
    assert {c["seq"] for c in cases} >= {0, 2**32 - 1, 2**64 - 1}
    assert len(IVS) == 2 and IVS[0] != IVS[1] and {c["iv"] for c in cases} == {0, 1}
    assert len(cases) == 30 and "OpenSSL" in DOC["source"]


@pytest.mark.parametrize("i", range(len(DOC["cases"])))
def test_nonce_ad_and_record_against_openssl_fixture(i):
    c = DOC["cases"][i]
    iv, seq, n = IVS[c["iv"]], c["seq"], c["n"]
    nonce = S.tls_nonce(iv, seq)
    ad = S.tls_ad(seq, n, *DOC["header"])
    assert nonce.hex() == c["nonce"] and ad.hex() == c["ad"] and len(nonce) == 12 and len(ad) == 13
    sealed = R.seal(KEY, nonce, R.data(n, b"rfc7905 pt %d" % n), ad)
    assert len(sealed) == n + 16
    assert hashlib.sha256(sealed[:-16]).hexdigest() == c["ct_sha256"] and sealed[-16:].hex() == c["tag"]


def test_nonce_rule_properties():
    iv = IVS[0]
    assert S.tls_nonce(iv, 0) == iv                                 # seq 0 leaves the IV
    for seq in (1, 2**32 - 1, 2**32, 2**64 - 1):
        nc = S.tls_nonce(iv, seq)
        assert nc[:4] == iv[:4]                                     # the padding touches no IV byte
        assert bytes(a ^ b for a, b in zip(nc[4:], iv[4:])) == struct.pack(">Q", seq)
    assert S.tls_nonce(b"\xff" * 12, 2**64 - 1) == b"\xff" * 4 + bytes(8)
    # the kernels' form: word 13 = le32(iv[0:4]), word 14 = le32(iv[4:8]) ^ bswap32(seq >> 32), word 15 likewise
    seq = 0x0102030405060708
    w = struct.unpack("<3I", S.tls_nonce(iv, seq))
    v = struct.unpack("<3I", iv)
    bswap = lambda x: struct.unpack("<I", struct.pack(">I", x))[0]  # noqa: E731
    assert w == (v[0], v[1] ^ bswap(seq >> 32), v[2] ^ bswap(seq & 0xFFFFFFFF))


def test_ad_default_header_is_tls12_application_data():
    assert S.tls_ad(5, 0x1234) == bytes(7) + b"\x05" + bytes([23, 3, 3, 0x12, 0x34])
    assert S.tls_ad(2**64 - 1, 16384, 22, 3, 1) == b"\xff" * 8 + bytes([22, 3, 1, 0x40, 0x00])


def test_live_openssl_agrees_where_it_loads():
    ossl = R.openssl()
    if ossl is None:
        pytest.skip("no libcrypto with ChaCha20-Poly1305")
    for iv in IVS:
        for seq, n in ((0, 0), (2**32, 17), (2**64 - 1, 1000)):
            nonce, ad = S.tls_nonce(iv, seq), S.tls_ad(seq, n)
            pt = R.data(n, b"live %d" % n)
            assert ossl.seal(KEY, nonce, pt, ad) == R.seal(KEY, nonce, pt, ad)
