"""CPU check of the bucket keying in TLS 1.3 form
(sg_wpr_keying_kernel<OPEN, true, Construction::kRfc8439, true>, suruga_amd/csrc/sg_wpr.hip).

A padded TLS 1.3 record of n = 64 k' inner bytes (4 KiB < n <= 16 KiB) has the MAC stream
AD(5) || 0^11 || n / 16 ciphertext blocks || le64(5) || le64(n): the RFC 8439 bucket
record's all-full-block stream (tests/test_wpr_bucket_model_rfc8439.py) behind another
AD.  wpr_geom<kRfc8439>(5, n) is the 13-byte AD's: o = 16, beta = 1, m = n / 16,
B = m + 2, rem = 16, delta = 0.  The constant term, restated here in Python integers:

* prefix: the block 17 03 03 be16(n + 16) and eleven zeros, at r^(m + 1) after the Horner
  step over the empty block beta, r^B in all;
* suffix: the one length block 5 + n 2^64 at weight r;
* pads 2^128 G(B), the i8 bias 128 G(m) A1 r over the record's own bytes and the
  accumulator seed: as in the RFC bucket model, from the same S(c) pieces.

That term plus the record kernel's MFMA part over the right-aligned frame must be
tests/rfc8439_ref.tag_of's tag under the TLS 1.3 header and nonce -- the tag
tests/tls13_ref.py puts behind such a record."""
from __future__ import annotations

import pytest

import rfc8439_ref as R
import rfc_batch_support as S
import test_wpr_bucket_model_rfc8439 as BM
import test_wpr_mac_model as M
import tls13_ref as T

P, N = M.P, M.N
BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)


def header(n: int) -> bytes:
    """The AD of a record of n inner bytes: opaque_type 23, 03 03, be16(fragment length)."""
    return bytes([0x17, 0x03, 0x03, (n + 16) >> 8, (n + 16) & 0xFF])


def constant_term_tls13(r: int, n: int) -> int:
    m = n // 16
    B = m + 2
    # G(m) and r^m from the table pieces the LIST keying builds (k' = 32 a + c)
    Rq, Tq = pow(r, 4, P), pow(r, 128, P)
    lo = [pow(Rq, b, P) for b in range(8)]
    hi = [pow(Rq, 8 * a, P) for a in range(4)]
    tk = [pow(Tq, k, P) for k in range(8)]
    sw = sum(lo) * sum(hi) % P
    kq = n >> 6
    ca, cl, ch = kq >> 5, kq & 7, (kq >> 3) & 3
    sc = (hi[ch] * sum(lo[:cl]) + sum(hi[:ch]) * sum(lo)) % P
    sk = (sw * sum(tk[:ca]) + pow(Tq, ca, P) * sc) % P
    g = sum(pow(r, e, P) for e in range(1, 5)) * sk % P
    rm = pow(Tq, ca, P) * hi[ch] * lo[cl] % P
    assert g == M.geo(r, m) and rm == pow(r, m, P)
    pads = (1 << 128) * (g + rm * M.geo(r, B - m))            # every block is full: rem = 16
    bias = g * sum(0x80 << (8 * k) for k in range(16)) * r     # sigma = 0, delta = 0
    seed = (P - ((1 << 24) * sum(1 << (8 * c) for c in range(32))) % P) % P * sw
    prefix = int.from_bytes(header(n) + bytes(11), "little") * pow(r, m + 1, P) * r  # block 0 of B + 1: weight r^(B)
    suffix = (5 + (n << 64)) * r
    return (pads + bias + seed + prefix + suffix) % P


def by_definition(r: int, n: int) -> int:
    """sum over the stream's non-ciphertext parts of value 2^.. r^(B - b), the i8 bias, minus the seed."""
    m = n // 16
    B = m + 2
    t = sum((1 << 128) * pow(r, B - b, P) for b in range(B))
    t += int.from_bytes(header(n) + bytes(11), "little") * pow(r, B, P)
    t += (5 + (n << 64)) * r
    t += sum(int.from_bytes(b"\x80" * 16, "little") * pow(r, B - 1 - c, P) for c in range(m))
    seed = (1 << 24) * sum(1 << (8 * c) for c in range(32)) * sum(pow(r, 4 * u, P) for u in range(32))
    return (t - seed) % P


def record(n: int, kslot: int, ct=None):
    key, iv = S.KEYS3[32 * kslot:32 * kslot + 32], S.IVS3[12 * kslot:12 * kslot + 12]
    seq = 2**32 - 2 + kslot
    nonce = T.nonce(iv, seq)
    r16, s16 = R.poly_key(key, nonce)
    ct = S.rnd(n, f"tls13 bucket model ct {n}") if ct is None else ct
    return key, nonce, ct, int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")


def frame_tag(monkeypatch, ad, ct, r, s, ctot) -> bytes:
    """The record kernel on the right-aligned record (frame bytes before it: i8 zeros) with the
    RFC bucket tables and this constant term."""
    n = len(ct)
    monkeypatch.setattr(M, "keying", lambda ad_, r_: dict(BM.keying_bucket(ad_, r_, n), ctot=ctot))
    return M.wpr_tag(ad, b"\x80" * (N - n) + ct, r, s)


def test_the_header_is_the_references():
    assert all(header(n) == T.header(n + 16) for n in BUCKET_NS)


@pytest.mark.parametrize("ff", [False, True], ids=["random", "all-ff"])
@pytest.mark.parametrize("n", BUCKET_NS)
def test_bucket_constant_term_and_tag(monkeypatch, n, ff):
    key, nonce, ct, r, s = record(n, (n // 64) % 3, b"\xff" * n if ff else None)
    ad = header(n)
    ctot = constant_term_tls13(r, n)
    assert ctot == by_definition(r, n)
    assert ctot == BM.keying_bucket(ad, r, n)["ctot"]  # the RFC bucket model agrees once it is given this AD
    assert frame_tag(monkeypatch, ad, ct, r, s, ctot) == R.tag_of(key, nonce, ad, ct)


def test_the_13_byte_ad_term_is_seen(monkeypatch):
    """The checker fails on the RFC 7905 constant term: prefix and length block differ."""
    n = 8256
    key, nonce, ct, r, s = record(n, 1)
    wrong = BM.keying_bucket(S.tls_ad(2**32 - 1, n), r, n)["ctot"]
    assert frame_tag(monkeypatch, header(n), ct, r, s, wrong) != R.tag_of(key, nonce, header(n), ct)
