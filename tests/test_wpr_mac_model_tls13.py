"""CPU check of the TLS 1.3 constant term of the wave-per-record keying kernel
(sg_wpr_keying_kernel<OPEN, false, Construction::kRfc8439, true>, suruga_amd/csrc/sg_wpr.hip).

A full TLS 1.3 record is 2^14 content bytes and the inner type byte, n = 2^14 + 1
(RFC 8446 section 5.2).  Its MAC stream is

    AD(5) || 11 zeros || 1024 ct blocks || [ct byte 2^14 || 15 zeros] || le64(5) || le64(n)

B = 1 + 1024 + 2 = 1027 blocks.  The record kernel runs the 1024 blocks as it does
for RFC 7905, with one block more behind them: delta = 1, rd[u] = r^(2 + u), so
ciphertext block m weighs r^(1026 - m).  The keying kernel restates the rest:

* pads: every block is full: 2^128 G(B);
* bias: 128 r^2 G(1024) A1 with A1 = sum_{k<16} 128 2^(8k);
* seed: as ever;
* prefix: the AD block (and the empty block the loop also steps) at r^1024 r^2 = r^(B - 0);
* tail: the tail ciphertext byte at r^2;
* suffix: le64(5) || le64(n) at r.

The MFMA part is tests/test_wpr_mac_model.py's at sigma = 0 with this keying; the tag
must equal tests/rfc8439_ref.tag_of over the 16385 ciphertext bytes."""
from __future__ import annotations

import numpy as np
import pytest

import rfc8439_ref as R
import test_wpr_mac_model as M
import tls13_ref as T

P, N = M.P, M.N
AD = T.header(N + 1 + 16)


def keying_tls13(tail: int):
    """M.keying's shape for the TLS 1.3 stream whose ciphertext byte 2^14 is `tail`."""

    def keying(ad: bytes, r: int) -> dict:
        assert ad == AD and len(ad) == 5
        beta, delta = 1, 1
        B = beta + 1024 + 2
        rd = [pow(r, 1 + delta + u, P) for u in range(5)]
        tk = [pow(r, 128 * k, P) for k in range(8)]
        Rq = pow(r, 4, P)
        lo = [pow(Rq, b, P) for b in range(8)]
        hi = [[pow(Rq, 8 * a, P) * (1 << (32 * h)) % P for a in range(4)] for h in range(2)]
        sw = sum(lo) * sum(hi[0]) % P
        g = sum(pow(r, e, P) for e in range(1, 5)) * sw * sum(tk) % P
        assert g == M.geo(r, 1024)
        gb = (g + pow(r, 1024, P) * M.geo(r, B - 1024)) % P
        pads = (1 << 128) * gb  # rem = 16: the last block's own term is p r = 0
        a1 = sum(0x80 << (8 * k) for k in range(16))
        bias = g * a1 * r * pow(r, delta, P)
        cj = (P - ((1 << 24) * sum(1 << (8 * c) for c in range(32))) % P) % P
        seed = cj * sw
        pre = ad + bytes(16 * beta - len(ad))
        hp = 0
        for b in range(beta + 1):  # block beta holds no prefix byte
            hp = (hp * r + int.from_bytes(pre[16 * b:16 * b + 16], "little")) % P
        prefix = hp * pow(r, 1024, P) * rd[0]
        suffix = tail * r * r + (len(ad) + ((N + 1) << 64)) * r
        ctot = (pads + bias + seed + prefix + suffix) % P
        return dict(sig=0, rd=rd, tk=tk, lo=lo, hi=hi, ctot=ctot)

    return keying


def constant_term_by_definition(tail: int, r: int) -> int:
    """The same term from the stream itself: every block's pad bit, the AD, tail and length
    blocks, the i8 bias of the 2^14 ciphertext bytes of the MFMA part, minus its seed."""
    B = 1027
    t = sum((1 << 128) * pow(r, B - b, P) for b in range(B))
    t += int.from_bytes(AD + bytes(11), "little") * pow(r, B, P)
    t += tail * pow(r, 2, P) + (5 + ((N + 1) << 64)) * r
    t += sum(int.from_bytes(b"\x80" * 16, "little") * pow(r, B - 1 - m, P) for m in range(1024))
    seed = (1 << 24) * sum(1 << (8 * c) for c in range(32)) * sum(pow(r, 4 * u, P) for u in range(32))
    return (t - seed) % P


def poly(key, nonce):
    r16, s16 = R.poly_key(key, nonce)
    return int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")


@pytest.mark.parametrize("tail", [0x00, 0x01, 0x80, 0xFF])
def test_tls13_constant_term_and_tag(monkeypatch, tail):
    rng = np.random.default_rng(8446 + tail)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ct = rng.bytes(N) + bytes([tail])
    r, s = poly(key, nonce)
    assert keying_tls13(tail)(AD, r)["ctot"] == constant_term_by_definition(tail, r)
    monkeypatch.setattr(M, "keying", keying_tls13(tail))
    assert M.wpr_tag(AD, ct[:N], r, s) == R.tag_of(key, nonce, AD, ct)


def test_all_ff_ciphertext(monkeypatch):
    rng = np.random.default_rng(13)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ct = b"\xff" * (N + 1)
    r, s = poly(key, nonce)
    monkeypatch.setattr(M, "keying", keying_tls13(0xFF))
    assert M.wpr_tag(AD, ct[:N], r, s) == R.tag_of(key, nonce, AD, ct)


def test_a_wrong_tail_weight_is_seen(monkeypatch):
    """The checker fails when the tail block sits one power off."""
    rng = np.random.default_rng(2)
    key, nonce = rng.bytes(32), rng.bytes(12)
    ct = rng.bytes(N) + b"\x5a"
    r, s = poly(key, nonce)

    def wrong(ad, r_):
        k = keying_tls13(0x5A)(ad, r_)
        k["ctot"] = (k["ctot"] + 0x5A * (r_ - r_ * r_)) % P
        return k

    monkeypatch.setattr(M, "keying", wrong)
    assert M.wpr_tag(AD, ct[:N], r, s) != R.tag_of(key, nonce, AD, ct)
