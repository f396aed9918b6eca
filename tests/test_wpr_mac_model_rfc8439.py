"""CPU check of the RFC 8439 constant term of the wave-per-record keying kernel
(sg_wpr_keying_kernel<OPEN, false, Construction::kRfc8439>, suruga_amd/csrc/sg_wpr.hip).

In the RFC stream ad || 0.. || ct || 0.. || le64(|ad|) || le64(n) the ciphertext
starts on a block boundary (o = 16 ceil(adlen / 16), sigma = 0, delta = 0), so the
MFMA part of the MAC is tests/test_wpr_mac_model.py's ciphertext term at sigma = 0,
unchanged; only the constant term differs:

* pads: every one of the B = beta + 1024 + 1 blocks is full (rem = 16): 2^128 G(B);
* bias: 128 G(1024) A1 r with A1 = sum_{k<16} 128 2^(8k) (sigma = 0: no A2 part);
* seed: as in the draft;
* prefix: ad and its zero padding, blocks 0..beta-1, Horner, times r^(1024 + 1)
  (the kernel's loop also steps the empty block beta, one factor r);
* suffix: the one full block le64(adlen) || le64(n), the stream's last, at weight r.

The existing model's ciphertext term is added (its keying() replaced by the one
below) and the tag compared with tests/rfc8439_ref.tag_of.  A wrong exponent in any
term shows here without a GPU."""
from __future__ import annotations

import numpy as np
import pytest

import rfc8439_ref as R
import test_wpr_mac_model as M

P, N = M.P, M.N
ADLENS = [0, 1, 5, 13, 15, 16, 17, 32, 255]


def keying_rfc(ad: bytes, r: int) -> dict:
    adlen = len(ad)
    o = -(-adlen // 16) * 16
    sig, beta = 0, o // 16
    B = beta + 1024 + 1
    rem, delta = 16, 0
    rd = [pow(r, 1 + delta + u, P) for u in range(5)]
    tk = [pow(r, 128 * k, P) for k in range(8)]
    Rq = pow(r, 4, P)
    lo = [pow(Rq, b, P) for b in range(8)]
    hi = [[pow(Rq, 8 * a, P) * (1 << (32 * h)) % P for a in range(4)] for h in range(2)]
    sw = sum(lo) * sum(hi[0]) % P
    g = sum(pow(r, e, P) for e in range(1, 5)) * sw * sum(tk) % P
    assert g == M.geo(r, 1024)
    gb = (g + pow(r, 1024, P) * M.geo(r, B - 1024)) % P
    pads = (1 << 128) * gb + ((1 << (8 * rem)) + P - (1 << 128)) * r  # the second term is p r = 0
    a1 = sum(0x80 << (8 * k) for k in range(16))
    bias = g * a1 * r
    cj = (P - ((1 << 24) * sum(1 << (8 * c) for c in range(32))) % P) % P
    seed = cj * sw
    pre = ad + bytes(o - adlen)
    hp = 0
    for b in range(beta + 1):  # block beta holds no prefix byte
        hp = (hp * r + int.from_bytes(pre[16 * b:16 * b + 16], "little")) % P
    prefix = hp * pow(r, 1024, P) * rd[0]
    suffix = (adlen + (N << 64)) * r
    ctot = (pads + bias + seed + prefix + suffix) % P
    return dict(sig=sig, rd=rd, tk=tk, lo=lo, hi=hi, ctot=ctot)


def constant_term_by_definition(ad: bytes, r: int) -> int:
    """The same term from the stream itself: every block's pad bit, the prefix and
    length blocks, the i8 bias of the ciphertext bytes, minus the accumulator seed."""
    beta = -(-len(ad) // 16)
    B = beta + 1024 + 1
    pre = ad + bytes(16 * beta - len(ad))
    t = sum((1 << 128) * pow(r, B - b, P) for b in range(B))
    t += sum(int.from_bytes(pre[16 * b:16 * b + 16], "little") * pow(r, B - b, P) for b in range(beta))
    t += (len(ad) + (N << 64)) * r
    t += sum(int.from_bytes(b"\x80" * 16, "little") * pow(r, B - beta - m, P) for m in range(1024))
    seed = (1 << 24) * sum(1 << (8 * c) for c in range(32)) * sum(pow(r, 4 * u, P) for u in range(32))
    return (t - seed) % P


@pytest.mark.parametrize("adlen", ADLENS)
def test_rfc_constant_term_and_tag(monkeypatch, adlen):
    rng = np.random.default_rng(8439 + adlen)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ad, ct = rng.bytes(adlen), rng.bytes(N)
    r16, s16 = R.poly_key(key, nonce)
    r, s = int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")
    assert keying_rfc(ad, r)["ctot"] == constant_term_by_definition(ad, r)
    monkeypatch.setattr(M, "keying", keying_rfc)
    assert M.wpr_tag(ad, ct, r, s) == R.tag_of(key, nonce, ad, ct)


def test_a_wrong_exponent_is_seen(monkeypatch):
    """The checker fails when the suffix sits one power off."""
    rng = np.random.default_rng(1)
    key, nonce, ad, ct = rng.bytes(32), rng.bytes(12), rng.bytes(13), rng.bytes(N)
    r16, s16 = R.poly_key(key, nonce)
    r, s = int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")

    def wrong(ad_, r_):
        k = keying_rfc(ad_, r_)
        k["ctot"] = (k["ctot"] + (len(ad_) + (N << 64)) * (r_ * r_ - r_)) % P
        return k

    monkeypatch.setattr(M, "keying", wrong)
    assert M.wpr_tag(ad, ct, r, s) != R.tag_of(key, nonce, ad, ct)
