"""The tests' RFC 8439 reference (tests/rfc8439_ref.py) against its three ties:
the stored OpenSSL vectors, OpenSSL live where libcrypto loads, and the draft
checker through the keystream the two constructions share.  CPU only."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import rfc8439_ref as ref


@pytest.fixture(scope="module")
def gold():
    return ref.golden()


def test_rfc8439_section_2_8_2_vector():
    """The RFC's own example (section 2.8.2)."""
    key = bytes(range(0x80, 0xA0))
    nonce = bytes.fromhex("070000004041424344454647")
    ad = bytes.fromhex("50515253c0c1c2c3c4c5c6c7")
    pt = (b"Ladies and Gentlemen of the class of '99: If I could offer you only one tip for the future, "
          b"sunscreen would be it.")
    out = ref.seal(key, nonce, pt, ad)
    assert out[:16].hex() == "d31a8d34648e60db7b86afbc53ef7ec2"
    assert out[-16:].hex() == "1ae10b594f09e26a7e902ecbd0600691"
    assert ref.open(key, nonce, out, ad) == (0, pt)
    assert ref.open(key, nonce, out, ad + b"\0")[0] == 1
    assert ref.open(key, nonce, out[:15], ad) == (2, b"")


def test_mac_stream_layout():
    for adlen, n in ((0, 0), (1, 0), (0, 1), (13, 17), (16, 16), (17, 31), (32, 64)):
        s = ref.mac_stream(bytes([7]) * adlen, bytes([9]) * n)
        P = -(-adlen // 16) * 16
        assert len(s) == ref.stream_len(n, adlen) and len(s) % 16 == 0
        assert s[:adlen] == bytes([7]) * adlen and s[adlen:P] == bytes(P - adlen)
        assert s[P:P + n] == bytes([9]) * n and s[P + n:-16] == bytes(len(s) - 16 - P - n)
        assert s[-16:] == adlen.to_bytes(8, "little") + n.to_bytes(8, "little")


def test_reproduces_every_small_vector(gold):
    assert len(gold["small"]) == len(ref.SMALL) ** 2
    assert {(v["n"], v["adlen"]) for v in gold["small"]} == {(n, a) for n in ref.SMALL for a in ref.SMALL}
    for v in gold["small"]:
        key, nonce, pt, ad = (bytes.fromhex(v[f]) for f in ("key", "nonce", "pt", "ad"))
        assert (key, nonce, pt, ad) == ref.single_message(v["n"], v["adlen"]), "the data rule moved"
        want = bytes.fromhex(v["ct_tag"])
        assert ref.seal(key, nonce, pt, ad) == want, (v["n"], v["adlen"])
        assert ref.open(key, nonce, want, ad) == (0, pt)


def test_reproduces_every_stored_shape(gold):
    """Every shape of the GPU tests: the golden file lists exactly those, and the
    reference gives OpenSSL's tag and ciphertext for each."""
    single = gold["shapes"]["single"]
    assert [(v["n"], v["adlen"]) for v in single] == ref.single_shapes() + [((1 << 20) + 7, 13)]
    assert bytes.fromhex(gold["key"]) == ref.KEY and bytes.fromhex(gold["nonce"]) == ref.NONCE
    for v in single:
        out = ref.sealed_single(v["n"], v["adlen"])
        assert out[-16:].hex() == v["tag"], (v["n"], v["adlen"])
        assert hashlib.sha256(out[:-16]).hexdigest() == v["ct_sha256"], (v["n"], v["adlen"])
    batch = gold["shapes"]["batch"]
    assert [(v["adlen"], v["n"]) for v in batch] == ref.batch_shapes()
    assert bytes.fromhex(gold["batch_keys"]) == ref.KEYS
    msgs = ref.batch_messages()
    assert len({m.nonce for m in msgs}) == len(msgs) and {m.kidx for m in msgs} == {0, 1, 2}
    for v, m in zip(batch, msgs):
        assert (m.kidx, m.nonce.hex()) == (v["key_index"], v["nonce"])
        assert m.sealed[-16:].hex() == v["tag"], v["index"]
        assert hashlib.sha256(m.sealed[:-16]).hexdigest() == v["ct_sha256"], v["index"]


def test_matches_openssl_live(gold):
    ossl = ref.openssl()
    if ossl is None:
        pytest.skip("libcrypto with ChaCha20-Poly1305 does not load here")
    rng = np.random.default_rng(8439)
    for _ in range(60):
        n, adlen = int(rng.integers(0, 5000)), int(rng.integers(0, 300))
        key, nonce, pt, ad = rng.bytes(32), rng.bytes(12), rng.bytes(n), rng.bytes(adlen)
        assert ref.seal(key, nonce, pt, ad) == ossl.seal(key, nonce, pt, ad), (n, adlen)
    n = (1 << 20) + 7
    key, nonce, pt, ad = rng.bytes(32), rng.bytes(12), rng.bytes(n), rng.bytes(13)
    assert ref.seal(key, nonce, pt, ad) == ossl.seal(key, nonce, pt, ad)


def test_keystream_is_the_draft_checkers_when_nonce_hi_is_zero(oracle):
    """Word 13 = 0 is the draft's state: same keystream, so the same ciphertext;
    only the MAC stream differs."""
    rng = np.random.default_rng(13)
    for n in (0, 1, 63, 64, 65, 1000, 3 * ref.TB + 5):
        key, nonce8, pt, ad = rng.bytes(32), rng.bytes(8), rng.bytes(n), rng.bytes(13)
        got = ref.seal(key, bytes(4) + nonce8, pt, ad)
        want = oracle.seal(key, nonce8, pt, ad)
        assert got[:n] == want[:n], n
        assert got[n:] != want[n:], n  # (the tags: different streams under the same r, s)
        # a non-zero word 13 is another keystream
        if n:
            assert ref.seal(key, b"\1\0\0\0" + nonce8, pt, ad)[:n] != want[:n]
