"""CPU check of the TLS 1.3 constant term of the wave-per-record keying kernel
(sg_wpr_keying_kernel<OPEN, false, Construction::kRfc8439, true>, suruga_amd/csrc/sg_wpr_keying.hip)
with the model of tests/wpr_model.py (keying(..., tail=)).

A full TLS 1.3 record is 2^14 content bytes and the inner type byte, n = 2^14 + 1
(RFC 8446 section 5.2).  Its MAC stream is

    AD(5) || 11 zeros || 1024 ct blocks || [ct byte 2^14 || 15 zeros] || le64(5) || le64(n)

B = 1 + 1024 + 2 = 1027 blocks.  The record kernel runs the 1024 blocks as it does
for RFC 7905, with one block more behind them: delta = 1, rd[u] = r^(2 + u), so
ciphertext block m weighs r^(1026 - m).  The keying kernel adds the tail ciphertext
byte at r^2 and the length block le64(5) || le64(n) at r.  keying()'s term must be
constant_term_by_definition()'s and the tag tests/rfc8439_ref.tag_of's over the 16385
ciphertext bytes."""
from __future__ import annotations

import numpy as np
import pytest

import rfc8439_ref as R
import tls13_ref as T
import wpr_model as W
from rfc_batch_support import poly_rs
from wpr_model import RFC8439, N, P

AD = T.header(N + 1 + 16)


@pytest.mark.parametrize("tail", [0x00, 0x01, 0x80, 0xFF])
def test_tls13_constant_term_and_tag(tail):
    rng = np.random.default_rng(8446 + tail)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ct = rng.bytes(N) + bytes([tail])
    r, s = poly_rs(key, nonce)
    kt = W.keying(RFC8439, AD, r, tail=tail)
    assert kt["ctot"] == W.constant_term_by_definition(RFC8439, AD, r, tail=tail)
    assert W.wpr_tag(AD, ct[:N], r, s, kt) == R.tag_of(key, nonce, AD, ct)


def test_all_ff_ciphertext():
    rng = np.random.default_rng(13)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ct = b"\xff" * (N + 1)
    r, s = poly_rs(key, nonce)
    assert W.wpr_tag(AD, ct[:N], r, s, W.keying(RFC8439, AD, r, tail=0xFF)) == R.tag_of(key, nonce, AD, ct)


def test_a_wrong_tail_weight_is_seen():
    """The checker fails when the tail block sits one power off."""
    rng = np.random.default_rng(2)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ct = rng.bytes(N) + b"\x5a"
    r, s = poly_rs(key, nonce)
    kt = W.keying(RFC8439, AD, r, tail=0x5A)
    assert W.wpr_tag(AD, ct[:N], r, s, kt) == R.tag_of(key, nonce, AD, ct)
    kt["ctot"] = (kt["ctot"] + 0x5A * (r - r * r)) % P
    assert W.wpr_tag(AD, ct[:N], r, s, kt) != R.tag_of(key, nonce, AD, ct)
