"""CPU check of the bucket keying in TLS 1.3 form
(sg_wpr_keying_kernel<OPEN, true, Construction::kRfc8439, true>, suruga_amd/csrc/sg_wpr_keying.hip)
with the model of tests/wpr_model.py.

A padded TLS 1.3 record of n = 64 k' inner bytes (4 KiB < n <= 16 KiB) has the MAC stream
AD(5) || 0^11 || n / 16 ciphertext blocks || le64(5) || le64(n): the RFC 8439 bucket
record's all-full-block stream (tests/test_wpr_bucket_model_rfc8439.py) behind another
AD, and wpr_geom<kRfc8439>(5, n) is the 13-byte AD's.  So the keying is the RFC bucket
keying given the 5-byte header: keying(RFC8439, header(n), r, n).  Its constant term
must be constant_term_by_definition()'s, and with the record kernel's part over the
right-aligned frame the tag must be tests/rfc8439_ref.tag_of's under the TLS 1.3 header
and nonce -- the tag tests/tls13_ref.py puts behind such a record."""
from __future__ import annotations

import pytest

import rfc8439_ref as R
import rfc_batch_support as S
import tls13_ref as T
import wpr_model as W
from wpr_model import RFC8439

BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)


def header(n: int) -> bytes:
    """The AD of a record of n inner bytes: opaque_type 23, 03 03, be16(fragment length)."""
    return bytes([0x17, 0x03, 0x03, (n + 16) >> 8, (n + 16) & 0xFF])


def record(n: int, kslot: int, ct=None):
    seq = 2**32 - 2 + kslot
    key, nonce, r, s = S.model_record(kslot, seq)
    assert nonce == T.nonce(S.IVS3[12 * kslot:12 * kslot + 12], seq)
    return key, nonce, S.rnd(n, f"tls13 bucket model ct {n}") if ct is None else ct, r, s


def test_the_header_is_the_references():
    assert all(header(n) == T.header(n + 16) for n in BUCKET_NS)


@pytest.mark.parametrize("ff", [False, True], ids=["random", "all-ff"])
@pytest.mark.parametrize("n", BUCKET_NS)
def test_bucket_constant_term_and_tag(n, ff):
    key, nonce, ct, r, s = record(n, (n // 64) % 3, b"\xff" * n if ff else None)
    ad = header(n)
    kt = W.keying(RFC8439, ad, r, n)
    assert kt["ctot"] == W.constant_term_by_definition(RFC8439, ad, r, n)
    assert kt["ctot"] == W.keying(RFC8439, T.header(n + 16), r, n)["ctot"]  # ... given the reference's header
    assert W.wpr_tag(ad, W.frame(ct), r, s, kt) == R.tag_of(key, nonce, ad, ct)


def test_the_13_byte_ad_term_is_seen():
    """The checker fails on the RFC 7905 constant term: prefix and length block differ."""
    n = 8256
    key, nonce, ct, r, s = record(n, 1)
    kt = W.keying(RFC8439, header(n), r, n)
    assert W.wpr_tag(header(n), W.frame(ct), r, s, kt) == R.tag_of(key, nonce, header(n), ct)
    wrong = dict(kt, ctot=W.keying(RFC8439, S.tls_ad(2**32 - 1, n), r, n)["ctot"])
    assert W.wpr_tag(header(n), W.frame(ct), r, s, wrong) != R.tag_of(key, nonce, header(n), ct)
