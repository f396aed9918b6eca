"""CPU check of the bucket keying in RFC 8439 form
(sg_wpr_keying_kernel<OPEN, true, Construction::kRfc8439>, suruga_amd/csrc/sg_wpr_keying.hip)
with the model of tests/wpr_model.py (keying(..., n)).

A bucket record of n = 64 k' bytes (4 KiB < n <= 16 KiB) runs right-aligned in the
record kernel's 16 KiB frame: the frame bytes before it enter the MFMA as i8 zeros,
so the record kernel's part is the full record's at sigma = 0 over the frame, and
only the constant term knows n.  wpr_geom<kRfc8439>(13, n): o = 16, beta = 1,
m = n / 16, B = m + 2, rem = 16, delta = 0; G(m) and r^m come from the S(c) pieces
of the tables (wpr_model's docstring).  keying()'s term must be
constant_term_by_definition()'s and the tag tests/rfc8439_ref.tag_of's for the TLS AD
and the RFC 7905 nonce."""
from __future__ import annotations

import pytest

import rfc8439_ref as R
import rfc_batch_support as S
import wpr_model as W
from wpr_model import RFC8439

BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)


def record(n: int, kslot: int):
    seq = 2**32 - 2 + kslot
    key, nonce, r, s = S.model_record(kslot, seq)
    return key, nonce, S.tls_ad(seq, n), S.rnd(n, f"bucket model ct {n}"), r, s


def frame_tag(ad, ct, r, s, **kw) -> bytes:
    return W.wpr_tag(ad, W.frame(ct), r, s, W.keying(RFC8439, ad, r, len(ct), **kw))


@pytest.mark.parametrize("n", BUCKET_NS)
def test_bucket_constant_term_and_tag(n):
    key, nonce, ad, ct, r, s = record(n, (n // 64) % 3)
    assert len(ad) == 13
    assert W.keying(RFC8439, ad, r, n)["ctot"] == W.constant_term_by_definition(RFC8439, ad, r, n)
    assert frame_tag(ad, ct, r, s) == R.tag_of(key, nonce, ad, ct)


def test_the_uniform_sums_are_seen_on_a_shorter_record():
    """The checker fails when a bucket record is keyed with the 16 KiB sums, and
    passes with them at n = 2^14."""
    key, nonce, ad, ct, r, s = record(8192, 1)
    assert frame_tag(ad, ct, r, s, uniform_sums=True) != R.tag_of(key, nonce, ad, ct)
    key, nonce, ad, ct, r, s = record(16384, 1)
    assert frame_tag(ad, ct, r, s, uniform_sums=True) == R.tag_of(key, nonce, ad, ct)
