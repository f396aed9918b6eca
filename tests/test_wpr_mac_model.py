"""CPU check of the decomposition behind the wave-per-record kernel's Poly1305
(sg_wpr_kernel in suruga_amd/csrc/sg_wpr.hip and sg_wpr_keying_kernel in sg_wpr_keying.hip),
draft form, with the model of tests/wpr_model.py: keying() for the keying kernel,
wpr_tag() for the record kernel on its 16 KiB frame.  The other record forms run the
same model: tests/test_wpr_mac_model_rfc8439.py, tests/test_wpr_mac_model_tls13.py,
tests/test_wpr_bucket_model_rfc8439.py, tests/test_wpr_bucket_model_tls13.py.

The model's tag must equal suruga's Poly1305 (poly1305.rs:195-315, through the
oracle) over the AEAD MAC stream ad || le64(|ad|) || ct || le64(|ct|)
(chacha20_poly1305.rs:19-42) for every AD length class the kernel takes
(sigma = (|ad| + 8) & 15, delta = 0 or 1), and for bucket records of
4 KiB < n <= 16 KiB, right-aligned in the frame behind i8 zeros.  keying()'s constant
term must be constant_term_by_definition(), which reads it off the stream and shares
no code with keying()."""
import struct

import numpy as np
import pytest

import wpr_model as W
from wpr_model import DRAFT, N

CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)


def tags(oracle, ad, ct, rk, sk):
    """(the model's tag, the oracle's) under the Poly1305 key rk || sk; the oracle clamps r (poly1305.rs:197-203)."""
    stream = ad + struct.pack("<Q", len(ad)) + ct + struct.pack("<Q", len(ct))  # chacha20_poly1305.rs:24-30
    r = int.from_bytes(rk, "little") & CLAMP
    kt = W.keying(DRAFT, ad, r, len(ct))
    assert kt["ctot"] == W.constant_term_by_definition(DRAFT, ad, r, len(ct))
    return W.wpr_tag(ad, W.frame(ct), r, int.from_bytes(sk, "little"), kt), oracle.poly1305(stream, rk, sk)


@pytest.mark.parametrize("adlen", [13, 0, 1, 7, 8, 24, 100, 255])
def test_wpr_decomposition_matches_reference_poly1305(oracle, adlen):
    rng = np.random.default_rng(1000 + adlen)
    ad = rng.bytes(adlen)
    ct = rng.bytes(N)
    got, want = tags(oracle, ad, ct, rng.bytes(16), rng.bytes(16))
    assert got == want


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_wpr_accumulator_bounds_extreme_bytes(oracle, fill):
    """All-zero and all-0xff ciphertext: the seeded accumulator stays in (0, 2^25)."""
    got, want = tags(oracle, bytes(13), bytes([fill]) * N, bytes([0xFF] * 16), bytes(16))
    assert got == want


@pytest.mark.parametrize("n", BUCKET_NS)
def test_draft_bucket_constant_term_and_tag(oracle, n):
    rng = np.random.default_rng(7539 + n)
    got, want = tags(oracle, oracle.tls_ad(2**32 - 2, n), rng.bytes(n), rng.bytes(16), rng.bytes(16))
    assert got == want
