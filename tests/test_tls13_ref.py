"""The TLS 1.3 record reference (tests/tls13_ref.py) against OpenSSL's records
(tests/golden/tls13_records.json, written by tests/golden/make_tls13_records.py),
and the rules of its open and strip.  CPU only."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import pytest

import rfc8439_ref as R
import tls13_ref as T

DOC = json.loads((Path(__file__).resolve().parent / "golden" / "tls13_records.json").read_text())
KEY = bytes.fromhex(DOC["key"])
IVS = [bytes.fromhex(x) for x in DOC["ivs"]]


def content(n: int) -> bytes:
    return R.data(n, b"tls13 content %d" % n)


def test_fixture_covers_the_edges():
    cases = DOC["cases"]
    assert {c["n"] for c in cases} == {0, 1, 15, 16, 100, 16384}
    assert {c["seq"] for c in cases} == {0, 2**32 - 1, 2**64 - 1}
    assert len(IVS) == 2 and IVS[1] == b"\xff" * 12 and {c["iv"] for c in cases} == {0, 1}
    assert {(c["n"], c["pad"]) for c in cases if c["pad"]} == {(100, 7)}
    assert len(cases) == 2 * 3 * 7 and "OpenSSL" in DOC["source"] and DOC["type"] == 23


@pytest.mark.parametrize("i", range(len(DOC["cases"])))
def test_nonce_header_and_record_against_openssl_fixture(i):
    c = DOC["cases"][i]
    iv, seq, n, pad = IVS[c["iv"]], c["seq"], c["n"], c["pad"]
    assert T.nonce(iv, seq).hex() == c["nonce"]
    assert T.header(n + 1 + pad + 16).hex() == c["ad"] and len(T.header(0)) == 5
    frag = T.seal(KEY, iv, seq, content(n), DOC["type"], pad)
    assert len(frag) == n + 1 + pad + 16
    assert hashlib.sha256(frag[:-16]).hexdigest() == c["ct_sha256"] and frag[-16:].hex() == c["tag"]
    st, inner, ty, cl = T.open(KEY, iv, seq, frag)
    assert (st, ty, cl) == (T.OK, 23, n) and inner == content(n) + b"\x17" + bytes(pad)


def test_strip_rules():
    assert T.strip(b"") is None and T.strip(bytes(5)) is None
    assert T.strip(b"\x17") == (0x17, 0)
    assert T.strip(b"abc\x16\0\0\0") == (0x16, 3)
    assert T.strip(b"ab\0\0\x17") == (0x17, 4)  # content that ends in zeros keeps them
    assert T.strip(b"\0\0\x15\0") == (0x15, 2)


def test_open_statuses():
    iv = IVS[0]
    frag = T.seal(KEY, iv, 5, b"hello", 22, pad=3)
    assert T.open(KEY, iv, 5, frag) == (T.OK, b"hello\x16\0\0\0", 22, 5)
    assert T.open(KEY, iv, 6, frag)[0] == T.BAD_MAC and T.open(KEY, iv, 6, frag)[2:] == (0, 0)
    bad = bytearray(frag)
    bad[-1] ^= 1
    assert T.open(KEY, iv, 5, bytes(bad))[0] == T.BAD_MAC
    assert T.open(KEY, iv, 5, frag[:15]) == (T.SHORT, b"", 0, 0)
    # a good tag over zeros alone, and over nothing: no type
    assert T.open(KEY, iv, 7, T.seal_inner(KEY, iv, 7, bytes(9))) == (T.NO_TYPE, bytes(9), 0, 0)
    assert T.open(KEY, iv, 8, T.seal_inner(KEY, iv, 8, b"")) == (T.NO_TYPE, b"", 0, 0)
    # the header is the additional data: a fragment cut by its padding no longer opens
    assert T.open(KEY, iv, 5, frag[:-17] + frag[-16:])[0] == T.BAD_MAC


def test_live_openssl_agrees_where_it_loads():
    ossl = R.openssl()
    if ossl is None:
        pytest.skip("no libcrypto with ChaCha20-Poly1305")
    for iv in IVS:
        for seq, n, pad in ((0, 0, 0), (2**32, 17, 1), (2**64 - 1, 1000, 255)):
            inner = T.inner(content(n), 23, pad)
            assert ossl.seal(KEY, T.nonce(iv, seq), inner, T.header(len(inner) + 16)) == T.seal(KEY, iv, seq, content(n), 23, pad)
