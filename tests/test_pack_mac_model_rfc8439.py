"""CPU check of the packed kernel's Poly1305 in RFC 8439 form
(sg_pack_kernel<OPEN, Construction::kRfc8439>, suruga_amd/csrc/sg_pack.hip).

A TLS record of n = 64 nb bytes has the MAC stream ad || 0^3 || ct || le64(13) ||
le64(n), B = 4 nb + 2 full blocks.  The kernel computes its accumulator as

    sum_j Q_j W(nb - 1 - j) + (block0 + 2^128) r^B + (lenblock + 2^128) r,

Q_j the four-step Horner of lane j's 64 ciphertext bytes (blocks 4 j + 1 .. 4 j + 4,
each with its pad bit), W(i) = r^(1 + 4 i) = hi[i >> 3] lo[i & 7] from the tables
hi[a] = r^(1 + 32 a), lo[b] = r^(4 b).  block0 is built as the kernel builds it:
from the byte-swapped sequence number, the header word and n -- not from the nonce
words, which under RFC 7905 carry the write IV.

The second half restates the kernel's word arithmetic (horner_step, words_to_f26,
mul_add of sg_device.h) to check the limb bounds of the unreduced accumulator that
sg_pack.hip's header comment derives for this stream."""
from __future__ import annotations

import struct

import pytest

import rfc8439_ref as R
import rfc_batch_support as S

P = S.P
M26, M32 = (1 << 26) - 1, (1 << 32) - 1
NBS = (1, 2, 7, 8, 9, 32, 33, 63, 64)
SEQ = 2**32 - 3  # + key index: crosses 2^32


def le_words(b: bytes):
    return list(struct.unpack("<%dI" % (len(b) // 4), b))


def bswap32(x: int) -> int:
    return int.from_bytes(struct.pack(">I", x & M32), "little")


def lane_q(block: bytes, r: int) -> int:
    h = 0
    for k in range(4):
        h = (h + int.from_bytes(block[16 * k:16 * k + 16], "little") + (1 << 128)) * r % P
    return h


def weight(i: int, r: int) -> int:
    hi = [pow(r, 1 + 32 * a, P) for a in range(8)]
    lo = [pow(r, 4 * b, P) for b in range(8)]
    return hi[i >> 3] * lo[i & 7] % P


def block0_words(seq: int, nonce12: bytes, n: int, hdr: int, ad_from_nonce: bool):
    """The kernel's four words of block 0.  ad_from_nonce: the draft's shortcut (its
    nonce is be64(seq), the AD's first eight bytes), wrong under RFC 7905."""
    if ad_from_nonce:
        _, a0, a1 = struct.unpack("<3I", nonce12)
    else:
        a0, a1 = bswap32(seq >> 32), bswap32(seq)
    return [a0, a1, (hdr & 0x00FFFFFF) | (((n >> 8) & 0xFF) << 24), n & 0xFF]


def packed_accumulator(r: int, seq: int, nonce12: bytes, ct: bytes, hdr=23 | 3 << 8 | 3 << 16, ad_from_nonce=False):
    n = len(ct)
    assert n % 64 == 0 and 64 <= n <= 4096
    nb = n // 64
    B = 4 * nb + 2
    rB = weight(nb - 1, r) * pow(r, 4, P) * r % P  # as the kernel: W(nb - 1) R r
    assert rB == pow(r, B, P)
    w = block0_words(seq, nonce12, n, hdr, ad_from_nonce)
    blk0 = sum(x << (32 * i) for i, x in enumerate(w)) + (1 << 128)
    sfx = 13 + (n << 64) + (1 << 128)
    acc = blk0 * rB + sfx * r
    for j in range(nb):
        acc += lane_q(ct[64 * j:64 * j + 64], r) * weight(nb - 1 - j, r)
    return acc % P


def record(nb: int, kslot: int, iv12: bytes):
    key = S.KEYS3[32 * kslot:32 * kslot + 32]
    seq = SEQ + kslot
    nonce = S.tls_nonce(iv12, seq)
    ct = S.rnd(64 * nb, f"pack model ct {nb} {kslot}")
    r16, s16 = R.poly_key(key, nonce)
    return key, seq, nonce, ct, int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")


@pytest.mark.parametrize("kslot", [0, 1, 2])
@pytest.mark.parametrize("nb", NBS)
def test_packed_decomposition_equals_the_reference(nb, kslot):
    key, seq, nonce, ct, r, s = record(nb, kslot, S.IVS3[12 * kslot:12 * kslot + 12])
    ad = S.tls_ad(seq, 64 * nb)
    acc = packed_accumulator(r, seq, nonce, ct)
    assert acc == S.accumulator(key, nonce, ad, ct)
    assert ((acc + s) % (1 << 128)).to_bytes(16, "little") == R.tag_of(key, nonce, ad, ct)


@pytest.mark.parametrize("nb", [1, 33])
def test_ad_words_from_the_nonce_are_wrong_unless_the_iv_is_zero(nb):
    """The model sees the trap: with a non-zero write IV the nonce words are not the
    AD's first eight bytes; with an all-zero IV they are, and the shortcut passes."""
    for iv, same in ((S.IVS3[12:24], False), (S.IVS3[:12], False), (bytes(12), True)):
        key, seq, nonce, ct, r, _ = record(nb, 1, iv)
        want = S.accumulator(key, nonce, S.tls_ad(seq, 64 * nb), ct)
        assert packed_accumulator(r, seq, nonce, ct) == want
        assert (packed_accumulator(r, seq, nonce, ct, ad_from_nonce=True) == want) == same


def test_a_wrong_length_block_is_seen():
    key, seq, nonce, ct, r, _ = record(7, 0, S.IVS3[:12])
    want = S.accumulator(key, nonce, S.tls_ad(seq, 448), ct)
    draft_suffix = (448 << 40) + (1 << 104)  # the draft's last block
    assert (packed_accumulator(r, seq, nonce, ct) - (13 + (448 << 64) + (1 << 128)) * r + draft_suffix * r) % P != want


# ---------------------------------------------------------------------------
# the kernel's word arithmetic and the bounds of the unreduced accumulator
# ---------------------------------------------------------------------------
def horner_step(h, m, pad, rw):
    """sg_device.h horner_step: h = (h + m + pad 2^128) r, h4 <= 4; every 64-bit column checked."""
    r0, r1, r2, r3 = rw
    s1, s2, s3 = r1 + (r1 >> 2), r2 + (r2 >> 2), r3 + (r3 >> 2)
    a, c = [0] * 5, 0
    for i in range(4):
        t = h[i] + m[i] + c
        a[i], c = t & M32, t >> 32
    a[4] = h[4] + pad + c
    assert a[4] <= 6
    d0 = a[0] * r0 + a[1] * s3 + a[2] * s2 + a[3] * s1
    d1 = a[0] * r1 + a[1] * r0 + a[2] * s3 + a[3] * s2 + a[4] * s1
    d2 = a[0] * r2 + a[1] * r1 + a[2] * r0 + a[3] * s3 + a[4] * s2
    d3 = a[0] * r3 + a[1] * r2 + a[2] * r1 + a[3] * r0 + a[4] * s3
    assert max(d0, d1, d2, d3) < 1 << 64
    t = (d1 & M32) + (d0 >> 32)
    e1, c = t & M32, t >> 32
    t = (d2 & M32) + (d1 >> 32) + c
    e2, c = t & M32, t >> 32
    t = (d3 & M32) + (d2 >> 32) + c
    e3, c = t & M32, t >> 32
    e4 = a[4] * r0 + (d3 >> 32) + c
    assert e4 < 1 << 32
    f, e4 = (e4 >> 2) * 5, e4 & 3
    out, c = [], 0
    for w in (d0 & M32, e1, e2, e3):
        t = w + (f if not out else 0) + c
        out.append(t & M32)
        c = t >> 32
    out.append(e4 + c)
    return out


def words_to_f26(w, hi):
    v = w[0] | w[1] << 32 | w[2] << 64 | w[3] << 96
    return [v & M26, (v >> 26) & M26, (v >> 52) & M26, (v >> 78) & M26, (w[3] >> 8) | (hi << 24)]


def limbs(x: int):
    return [(x >> (26 * i)) & M26 for i in range(5)]


def value(f) -> int:
    return sum(x << (26 * i) for i, x in enumerate(f))


def mul_add(a, b, c):
    """sg_device.h mul_add: a b + c with one carry pass; every column below 2^64, every carry a word."""
    s = [x * 5 for x in b]
    assert max(s) < 1 << 32
    cols = [
        a[0] * b[0] + a[1] * s[4] + a[2] * s[3] + a[3] * s[2] + a[4] * s[1],
        a[0] * b[1] + a[1] * b[0] + a[2] * s[4] + a[3] * s[3] + a[4] * s[2],
        a[0] * b[2] + a[1] * b[1] + a[2] * b[0] + a[3] * s[4] + a[4] * s[3],
        a[0] * b[3] + a[1] * b[2] + a[2] * b[1] + a[3] * b[0] + a[4] * s[4],
        a[0] * b[4] + a[1] * b[3] + a[2] * b[2] + a[3] * b[1] + a[4] * b[0],
    ]
    h, cy = [], 0
    for i in range(5):
        assert c[i] + cy < 1 << 32
        d = c[i] + cy + cols[i]
        assert d < 1 << 64
        h.append(d & M26)
        cy = d >> 26
        assert cy < 1 << 32
    e = h[0] + cy * 5
    h[0] = e & M26
    h[1] += e >> 26
    return h


def carry1(f):
    f = list(f)
    for i in range(4):
        f[i + 1] += f[i] >> 26
        f[i] &= M26
    f[0] += (f[4] >> 26) * 5
    f[4] &= M26
    f[1] += f[0] >> 26
    f[0] &= M26
    return f


@pytest.mark.parametrize("rbytes", [b"\xff" * 16, None], ids=["r all ones", "r drawn"])
@pytest.mark.parametrize("fill", [0xFF, 0x00, None], ids=["ct 0xff", "ct 0x00", "ct drawn"])
def test_limb_bounds_of_64_terms(rbytes, fill):
    """A 4096-byte record (64 lane terms), all-0xff ciphertext among the fills, r with
    every clamped bit set among the keys: the bounds of sg_pack.hip's header comment
    hold term by term and for the sums, and the finish gives the stream's accumulator."""
    r = int.from_bytes(rbytes or S.rnd(16, "pack bound r"), "little") & R.CLAMP
    rw = le_words(r.to_bytes(16, "little"))
    nb = 64
    ct = bytes([fill]) * (64 * nb) if fill is not None else S.rnd(64 * nb, "pack bound ct")
    acc = [0, 0, 0, 0, 0]  # the three LDS words: (v0, v2), (v3, v4) halves and v1 as 64 bits
    for j in range(nb):
        d = le_words(ct[64 * j:64 * j + 64])
        h = [0] * 5
        for k in range(4):
            h = horner_step(h, d[4 * k:4 * k + 4], 1, rw)
            assert h[4] <= 4
        Q = words_to_f26(h[:4], h[4])
        assert max(Q[:4]) < 1 << 26 and Q[4] < 1 << 27
        assert value(Q) % P == lane_q(ct[64 * j:64 * j + 64], r)
        i = nb - 1 - j
        W = mul_add(limbs(pow(r, 1 + 32 * (i >> 3), P)), limbs(pow(r, 4 * (i & 7), P)), [0] * 5)
        t = mul_add(Q, W, [0] * 5)
        assert t[0] < 1 << 26 and t[1] < (1 << 26) + (1 << 7) and max(t[2:]) < 1 << 26
        assert value(t) % P == lane_q(ct[64 * j:64 * j + 64], r) * weight(i, r) % P
        acc = [x + y for x, y in zip(acc, t)]
    # a half of a 64-bit atomic never carries into the other; limb 1 has its own word
    assert max(acc[0], acc[2], acc[3], acc[4]) < 1 << 32 and acc[1] < (1 << 32) + (1 << 13)
    # finish (pack_run): carry1 of the low words, limb 1's bit 32 into limb 2, the constant term
    lo1, hi1 = acc[1] & M32, acc[1] >> 32
    assert hi1 <= 1
    f = carry1([acc[0], lo1, acc[2], acc[3], acc[4]])
    f[2] += hi1 << 6
    w0 = block0_words(SEQ, bytes(12), 64 * nb, 23 | 3 << 8 | 3 << 16, False)
    rB = pow(r, 4 * nb + 2, P)
    ctot = mul_add(words_to_f26(w0, 1), limbs(rB), mul_add(words_to_f26([13, 0, 64 * nb, 0], 1), limbs(r), [0] * 5))
    f = carry1([x + y for x, y in zip(f, ctot)])
    assert max(f) < (1 << 26) + (1 << 8)
    assert value(f) % P == packed_accumulator(r, SEQ, bytes(12), ct)


def test_the_carry_bound_by_reasoning():
    """Limb 1 of a mul_add result is below 2^26 + 2^7 for every operand in bounds: the
    last column has no factor 5, so with a_i < 2^26 (a_4 < 2^27) and b_i < 2^26 + 2^8
    its carry is below 7 2^26, and 5 times that plus limb 0 carries at most 35 < 2^7."""
    b = (1 << 26) + (1 << 8)
    col4 = 4 * (1 << 26) * b + (1 << 27) * b + (1 << 32)
    assert ((col4 >> 26) * 5 + M26) >> 26 < 1 << 7
