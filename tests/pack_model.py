"""Python model of the packed kernel's Poly1305 (sg_pack_kernel<OPEN, Construction::kRfc8439>
and its TLS 1.3 form, suruga_amd/csrc/sg_pack.hip) -- TEST INFRASTRUCTURE ONLY;
tests/test_pack_mac_model_rfc8439.py and tests/test_pack_mac_model_tls13.py hold it
against the references.

A record of n = 64 nb ciphertext bytes has the MAC stream block0 || ct || length block,
B = 4 nb + 2 full blocks:

* RFC7905: block0 = the 13-byte TLS AD and three zeros, length block le64(13) || le64(n);
* TLS13:   block0 = the header 17 03 03 be16(n + 16) and eleven zeros, le64(5) || le64(n).

The kernel computes its accumulator as

    sum_j Q_j W(nb - 1 - j) + (block0 + 2^128) r^B + (length block + 2^128) r,

Q_j the four-step Horner of lane j's 64 ciphertext bytes (blocks 4 j + 1 .. 4 j + 4,
each with its pad bit), W(i) = r^(1 + 4 i) = hi[i >> 3] lo[i & 7] from the tables
hi[a] = r^(1 + 32 a), lo[b] = r^(4 b).  block0 is built as the kernel builds it: under
RFC 7905 from the byte-swapped sequence number, the header word and n -- not from the
nonce words, which carry the write IV -- and under TLS 1.3 from n alone.

The second half restates the kernel's word arithmetic (horner_step, words_to_f26,
mul_add, carry1 of sg_device.h); every bound that sg_pack.hip's header comment derives
for a column, a carry or a step is asserted inside it, and limb_walk runs one record
through it.

Imports without torch and without the native library."""
from __future__ import annotations

import struct

P = (1 << 130) - 5
M26, M32 = (1 << 26) - 1, (1 << 32) - 1
RFC7905, TLS13 = "rfc7905", "tls13"
ADLEN = {RFC7905: 13, TLS13: 5}
HDR = 23 | 3 << 8 | 3 << 16  # application_data, version 3.3


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


def block0_words(form: str, n: int, seq: int = 0, nonce12: bytes = bytes(12), hdr: int = HDR, ad_from_nonce: bool = False):
    """The kernel's four words of block 0.  TLS13: 17 03 03 be16(L), L = n + 16, eleven
    zero bytes.  RFC7905: the AD; ad_from_nonce is the draft's shortcut (its nonce is
    be64(seq), the AD's first eight bytes), wrong under RFC 7905."""
    if form == TLS13:
        L = n + 16
        return [0x00030317 | ((L >> 8) << 24), L & 0xFF, 0, 0]
    if ad_from_nonce:
        _, a0, a1 = struct.unpack("<3I", nonce12)
    else:
        a0, a1 = bswap32(seq >> 32), bswap32(seq)
    return [a0, a1, (hdr & 0x00FFFFFF) | (((n >> 8) & 0xFF) << 24), n & 0xFF]


def length_block(form: str, n: int) -> int:
    return ADLEN[form] + (n << 64)


def constant_term(form: str, r: int, nb: int, **block0) -> int:
    """(block0 + 2^128) r^B + (length block + 2^128) r; block0: block0_words' keywords."""
    n = 64 * nb
    rB = weight(nb - 1, r) * pow(r, 4, P) * r % P  # as the kernel: W(nb - 1) R r
    assert rB == pow(r, 4 * nb + 2, P)
    blk0 = sum(x << (32 * i) for i, x in enumerate(block0_words(form, n, **block0))) + (1 << 128)
    return (blk0 * rB + (length_block(form, n) + (1 << 128)) * r) % P


def packed_accumulator(form: str, r: int, ct: bytes, **block0) -> int:
    nb = len(ct) // 64
    assert len(ct) % 64 == 0 and 1 <= nb <= 64
    acc = constant_term(form, r, nb, **block0)
    for j in range(nb):
        acc += lane_q(ct[64 * j:64 * j + 64], r) * weight(nb - 1 - j, r)
    return acc % P


# ---------------------------------------------------------------------------
# the kernel's word arithmetic
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


def limb_walk(form: str, r: int, ct: bytes, **block0) -> None:
    """The kernel's words on one record, step by step: the bounds of sg_pack.hip's header
    comment hold term by term and for the sums, every term is its lane's, and the finish
    with the form's constant term gives the stream's accumulator.  Asserts all of it."""
    rw = le_words(r.to_bytes(16, "little"))
    n, nb = len(ct), len(ct) // 64
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
    blk0 = words_to_f26(block0_words(form, n, **block0), 1)
    sfx = words_to_f26([ADLEN[form], 0, n, 0], 1)
    assert max(blk0) < 1 << 27 and max(sfx) < 1 << 27  # mul_add's operand bound
    ctot = mul_add(blk0, limbs(pow(r, 4 * nb + 2, P)), mul_add(sfx, limbs(r), [0] * 5))
    assert value(ctot) % P == constant_term(form, r, nb, **block0)
    f = carry1([x + y for x, y in zip(f, ctot)])
    assert max(f) < (1 << 26) + (1 << 8)
    assert value(f) % P == packed_accumulator(form, r, ct, **block0)
