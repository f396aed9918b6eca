"""CPU check of the RFC 8439 constant term of the wave-per-record keying kernel
(sg_wpr_keying_kernel<OPEN, false, Construction::kRfc8439>, suruga_amd/csrc/sg_wpr_keying.hip)
with the model of tests/wpr_model.py.

In the RFC stream ad || 0.. || ct || 0.. || le64(|ad|) || le64(n) the ciphertext
starts on a block boundary (o = 16 ceil(adlen / 16), sigma = 0, delta = 0) and every
one of the B = beta + 1024 + 1 blocks is full, so the record kernel's part is the
draft's at sigma = 0 and only the constant term differs: no A2 part of the bias, the
prefix ad and its zero padding, the suffix the one block le64(adlen) || le64(n) at
weight r.  keying()'s term must be constant_term_by_definition()'s and the tag
tests/rfc8439_ref.tag_of's.  A wrong exponent in any term shows here without a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import rfc8439_ref as R
import wpr_model as W
from rfc_batch_support import poly_rs
from wpr_model import RFC8439, N, P

ADLENS = [0, 1, 5, 13, 15, 16, 17, 32, 255]


@pytest.mark.parametrize("adlen", ADLENS)
def test_rfc_constant_term_and_tag(adlen):
    rng = np.random.default_rng(8439 + adlen)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ad, ct = rng.bytes(adlen), rng.bytes(N)
    r, s = poly_rs(key, nonce)
    kt = W.keying(RFC8439, ad, r)
    assert kt["ctot"] == W.constant_term_by_definition(RFC8439, ad, r)
    assert W.wpr_tag(ad, ct, r, s, kt) == R.tag_of(key, nonce, ad, ct)


def test_a_wrong_exponent_is_seen():
    """The checker fails when the suffix sits one power off."""
    rng = np.random.default_rng(1)
    key, nonce, ad, ct = rng.bytes(32), rng.bytes(12), rng.bytes(13), rng.bytes(N)
    r, s = poly_rs(key, nonce)
    kt = W.keying(RFC8439, ad, r)
    assert W.wpr_tag(ad, ct, r, s, kt) == R.tag_of(key, nonce, ad, ct)
    kt["ctot"] = (kt["ctot"] + (len(ad) + (N << 64)) * (r * r - r)) % P
    assert W.wpr_tag(ad, ct, r, s, kt) != R.tag_of(key, nonce, ad, ct)
