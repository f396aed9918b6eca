"""CPU check of the packed kernel's Poly1305 in TLS 1.3 form
(sg_pack_kernel<OPEN, Construction::kRfc8439, true>, suruga_amd/csrc/sg_pack.hip).

A TLS 1.3 record whose inner plaintext is n = 64 nb bytes has the MAC stream
AD(5) || 0^11 || ct || le64(5) || le64(n), B = 4 nb + 2 full blocks, the AD the record
header 17 03 03 be16(n + 16).  The kernel computes its accumulator as

    sum_j Q_j W(nb - 1 - j) + (block0 + 2^128) r^B + (5 + n 2^64 + 2^128) r,

lane terms, weights and tables those of the RFC form (tests/test_pack_mac_model_rfc8439.py,
whose restatement of the kernel's word arithmetic is imported, not copied); block0 is
built as the kernel builds it, from n alone.  The tag must be the reference's for
tests/tls13_ref.py's header, and the limb bounds that sg_pack.hip's header comment
derives for the RFC stream must hold for this one, all-0xff ciphertext included."""
from __future__ import annotations

import pytest

import rfc8439_ref as R
import rfc_batch_support as S
import test_pack_mac_model_rfc8439 as M
import tls13_ref as T

P = S.P
NBS = (1, 2, 33, 64)
SEQ = 2**32 - 3


def block0_words(n: int):
    """The kernel's four words of block 0: 17 03 03 be16(L), L = n + 16, eleven zero bytes."""
    L = n + 16
    return [0x00030317 | ((L >> 8) << 24), L & 0xFF, 0, 0]


def constant_term(r: int, nb: int) -> int:
    n = 64 * nb
    rB = M.weight(nb - 1, r) * pow(r, 4, P) * r % P  # as the kernel: W(nb - 1) R r
    assert rB == pow(r, 4 * nb + 2, P)
    blk0 = sum(x << (32 * i) for i, x in enumerate(block0_words(n))) + (1 << 128)
    return (blk0 * rB + (5 + (n << 64) + (1 << 128)) * r) % P


def packed_accumulator(r: int, ct: bytes) -> int:
    nb = len(ct) // 64
    assert len(ct) % 64 == 0 and 1 <= nb <= 64
    acc = constant_term(r, nb)
    for j in range(nb):
        acc += M.lane_q(ct[64 * j:64 * j + 64], r) * M.weight(nb - 1 - j, r)
    return acc % P


def record(nb: int, kslot: int, fill):
    key, iv = S.KEYS3[32 * kslot:32 * kslot + 32], S.IVS3[12 * kslot:12 * kslot + 12]
    nonce = T.nonce(iv, SEQ + kslot)
    ct = bytes([fill]) * (64 * nb) if fill is not None else S.rnd(64 * nb, f"pack13 model ct {nb} {kslot}")
    r16, s16 = R.poly_key(key, nonce)
    return key, nonce, ct, int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")


def test_block0_is_the_record_header():
    for n in (64, 192, 240, 4096):
        w = block0_words(n)
        assert b"".join(x.to_bytes(4, "little") for x in w) == T.header(n + 16) + bytes(11)


@pytest.mark.parametrize("fill", [None, 0xFF], ids=["ct drawn", "ct 0xff"])
@pytest.mark.parametrize("kslot", [0, 1, 2])
@pytest.mark.parametrize("nb", NBS)
def test_packed_decomposition_equals_the_reference(nb, kslot, fill):
    key, nonce, ct, r, s = record(nb, kslot, fill)
    ad = T.header(64 * nb + 16)
    acc = packed_accumulator(r, ct)
    assert acc == S.accumulator(key, nonce, ad, ct)
    assert ((acc + s) % (1 << 128)).to_bytes(16, "little") == R.tag_of(key, nonce, ad, ct)


def test_the_rfc7905_constant_term_is_seen():
    """The 13-byte AD's constant term (or its length block alone) gives another accumulator."""
    key, nonce, ct, r, _ = record(7, 0, None)
    want = S.accumulator(key, nonce, T.header(448 + 16), ct)
    assert packed_accumulator(r, ct) == want
    assert M.packed_accumulator(r, SEQ, nonce, ct) != want
    assert (packed_accumulator(r, ct) + (13 - 5) * r) % P != want


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("rbytes", [b"\xff" * 16, None], ids=["r all ones", "r drawn"])
@pytest.mark.parametrize("fill", [0xFF, None], ids=["ct 0xff", "ct drawn"])
def test_limb_bounds_along_the_kernel_arithmetic(nb, rbytes, fill):
    """The kernel's words, step by step (horner_step, words_to_f26, mul_add, carry1 as
    restated for the RFC form): every bound of sg_pack.hip's header comment is asserted
    on the way, and the finish with this stream's constant term gives its accumulator."""
    r = int.from_bytes(rbytes or S.rnd(16, "pack13 bound r"), "little") & R.CLAMP
    rw = M.le_words(r.to_bytes(16, "little"))
    ct = bytes([fill]) * (64 * nb) if fill is not None else S.rnd(64 * nb, f"pack13 bound ct {nb}")
    acc = [0] * 5
    for j in range(nb):
        d = M.le_words(ct[64 * j:64 * j + 64])
        h = [0] * 5
        for k in range(4):
            h = M.horner_step(h, d[4 * k:4 * k + 4], 1, rw)
            assert h[4] <= 4
        Q = M.words_to_f26(h[:4], h[4])
        assert max(Q[:4]) < 1 << 26 and Q[4] < 1 << 27
        i = nb - 1 - j
        W = M.mul_add(M.limbs(pow(r, 1 + 32 * (i >> 3), P)), M.limbs(pow(r, 4 * (i & 7), P)), [0] * 5)
        t = M.mul_add(Q, W, [0] * 5)
        assert t[0] < 1 << 26 and t[1] < (1 << 26) + (1 << 7) and max(t[2:]) < 1 << 26
        acc = [x + y for x, y in zip(acc, t)]
    assert max(acc[0], acc[2], acc[3], acc[4]) < 1 << 32 and acc[1] < (1 << 32) + (1 << 13)
    lo1, hi1 = acc[1] & M.M32, acc[1] >> 32
    assert hi1 <= 1
    f = M.carry1([acc[0], lo1, acc[2], acc[3], acc[4]])
    f[2] += hi1 << 6
    n = 64 * nb
    blk0, sfx = M.words_to_f26(block0_words(n), 1), M.words_to_f26([5, 0, n, 0], 1)
    assert max(blk0) < 1 << 27 and max(sfx) < 1 << 27  # mul_add's operand bound
    ctot = M.mul_add(blk0, M.limbs(pow(r, 4 * nb + 2, P)), M.mul_add(sfx, M.limbs(r), [0] * 5))
    assert M.value(ctot) % P == constant_term(r, nb)
    f = M.carry1([x + y for x, y in zip(f, ctot)])
    assert max(f) < (1 << 26) + (1 << 8)
    assert M.value(f) % P == packed_accumulator(r, ct)
