"""CPU check of the bucket keying in RFC 8439 form
(sg_wpr_keying_kernel<OPEN, true, Construction::kRfc8439>, suruga_amd/csrc/sg_wpr.hip).

A bucket record of n = 64 k' bytes (4 KiB < n <= 16 KiB) runs right-aligned in the
record kernel's 16 KiB frame: the frame bytes before it enter the MFMA as i8 zeros,
so the ciphertext term is tests/test_wpr_mac_model.py's at sigma = 0 over the frame,
and only the constant term knows n.  With wpr_geom<kRfc8439>(13, n): o = 16,
beta = 1, m = n / 16, B = m + 2, rem = 16, delta = 0, and as the kernel builds them
from its tables (k' = 32 a + c, R = r^4, T = r^128):

    S(c)  = sum_{a' < c >> 3} R^(8 a') sum_b R^b + R^(8 (c >> 3)) sum_{b < c & 7} R^b
    S(k') = SW sum_{k < a} T^k + T^a S(c)
    G(m)  = (r + r^2 + r^3 + r^4) S(k'),   r^m = T^a R^(8 (c >> 3)) R^(c & 7)

* pads: 2^128 G(B), G(B) = G(m) + r^m G(2);
* bias: 128 G(m) A1 r over the record's own bytes; seed as in the draft;
* prefix: the AD and three zero bytes (then the empty block beta), times r^m r;
* suffix: the one full block le64(13) || le64(n) at weight r.

The tag must be tests/rfc8439_ref.tag_of's for the TLS AD and the RFC 7905 nonce."""
from __future__ import annotations

import pytest

import rfc8439_ref as R
import rfc_batch_support as S
import test_wpr_mac_model as M

P, N = M.P, M.N
BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)


def keying_bucket(ad: bytes, r: int, n: int, uniform_sums: bool = False) -> dict:
    adlen = len(ad)
    o = -(-adlen // 16) * 16
    beta, m = o // 16, n // 16
    B = beta + m + 1
    rd = [pow(r, 1 + u, P) for u in range(5)]
    T = pow(r, 128, P)
    tk = [pow(T, k, P) for k in range(8)]
    Rq = pow(r, 4, P)
    lo = [pow(Rq, b, P) for b in range(8)]
    hi = [[pow(Rq, 8 * a, P) * (1 << (32 * h)) % P for a in range(4)] for h in range(2)]
    sw = sum(lo) * sum(hi[0]) % P
    g4 = sum(pow(r, e, P) for e in range(1, 5))
    kq = n >> 6
    ca, cl, ch = kq >> 5, kq & 7, (kq >> 3) & 3
    plo, xlo = sum(lo[:cl]), lo[cl]
    phi, yc = sum(hi[0][:ch]), hi[0][ch]
    pta, ta = sum(tk[:ca]), pow(T, ca, P)
    sc = (yc * plo + phi * sum(lo)) % P
    sk = (sw * pta + ta * sc) % P
    g, rm = g4 * sk % P, ta * yc * xlo % P
    if uniform_sums:  # the uniform launch's sums: right for n = 2^14 only
        g, rm = g4 * sw * sum(tk) % P, pow(T, 8, P)
    else:
        assert g == M.geo(r, m) and rm == pow(r, m, P)
    gb = (g + rm * M.geo(r, B - m)) % P
    pads = (1 << 128) * gb + ((1 << 128) + P - (1 << 128)) * r
    bias = g * sum(0x80 << (8 * k) for k in range(16)) * r
    seed = (P - ((1 << 24) * sum(1 << (8 * c) for c in range(32))) % P) % P * sw
    pre = ad + bytes(o - adlen)
    hp = 0
    for b in range(beta + 1):  # block beta holds no prefix byte
        hp = (hp * r + int.from_bytes(pre[16 * b:16 * b + 16], "little")) % P
    prefix = hp * rm * rd[0]
    suffix = (adlen + (n << 64)) * r
    return dict(sig=0, rd=rd, tk=tk, lo=lo, hi=hi, ctot=(pads + bias + seed + prefix + suffix) % P)


def constant_term_by_definition(ad: bytes, r: int, n: int) -> int:
    beta, m = -(-len(ad) // 16), n // 16
    B = beta + m + 1
    pre = ad + bytes(16 * beta - len(ad))
    t = sum((1 << 128) * pow(r, B - b, P) for b in range(B))
    t += sum(int.from_bytes(pre[16 * b:16 * b + 16], "little") * pow(r, B - b, P) for b in range(beta))
    t += (len(ad) + (n << 64)) * r
    t += sum(int.from_bytes(b"\x80" * 16, "little") * pow(r, B - beta - c, P) for c in range(m))
    seed = (1 << 24) * sum(1 << (8 * c) for c in range(32)) * sum(pow(r, 4 * u, P) for u in range(32))
    return (t - seed) % P


def record(n: int, kslot: int):
    key, iv = S.KEYS3[32 * kslot:32 * kslot + 32], S.IVS3[12 * kslot:12 * kslot + 12]
    seq = 2**32 - 2 + kslot
    nonce, ad = S.tls_nonce(iv, seq), S.tls_ad(seq, n)
    r16, s16 = R.poly_key(key, nonce)
    return key, nonce, ad, S.rnd(n, f"bucket model ct {n}"), int.from_bytes(r16, "little") & R.CLAMP, \
        int.from_bytes(s16, "little")


def frame_tag(monkeypatch, ad, ct, r, s, **kw) -> bytes:
    """The record kernel on the right-aligned record: frame bytes before it are i8 zeros (0x80)."""
    n = len(ct)
    monkeypatch.setattr(M, "keying", lambda ad_, r_: keying_bucket(ad_, r_, n, **kw))
    return M.wpr_tag(ad, b"\x80" * (N - n) + ct, r, s)


@pytest.mark.parametrize("n", BUCKET_NS)
def test_bucket_constant_term_and_tag(monkeypatch, n):
    key, nonce, ad, ct, r, s = record(n, (n // 64) % 3)
    assert len(ad) == 13
    assert keying_bucket(ad, r, n)["ctot"] == constant_term_by_definition(ad, r, n)
    assert frame_tag(monkeypatch, ad, ct, r, s) == R.tag_of(key, nonce, ad, ct)


def test_the_uniform_sums_are_seen_on_a_shorter_record(monkeypatch):
    """The checker fails when a bucket record is keyed with the 16 KiB sums, and
    passes with them at n = 2^14."""
    key, nonce, ad, ct, r, s = record(8192, 1)
    assert frame_tag(monkeypatch, ad, ct, r, s, uniform_sums=True) != R.tag_of(key, nonce, ad, ct)
    key, nonce, ad, ct, r, s = record(16384, 1)
    assert frame_tag(monkeypatch, ad, ct, r, s, uniform_sums=True) == R.tag_of(key, nonce, ad, ct)
