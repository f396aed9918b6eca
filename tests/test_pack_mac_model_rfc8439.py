"""CPU check of the packed kernel's Poly1305 in RFC 8439 form
(sg_pack_kernel<OPEN, Construction::kRfc8439>, suruga_amd/csrc/sg_pack.hip) with the
model of tests/pack_model.py, form RFC7905.

A TLS record of n = 64 nb bytes has the MAC stream ad || 0^3 || ct || le64(13) ||
le64(n), B = 4 nb + 2 full blocks.  The model's decomposition into lane terms, weights
and the constant term must give tests/rfc8439_ref.py's accumulator and tag; block0 must
come from the sequence number, not from the nonce words, which under RFC 7905 carry
the write IV; and along the kernel's word arithmetic (pack_model.limb_walk) the limb
bounds of the unreduced accumulator that sg_pack.hip's header comment derives must hold."""
from __future__ import annotations

import pytest

import pack_model as M
import rfc8439_ref as R
import rfc_batch_support as S
from pack_model import RFC7905

P = M.P
NBS = (1, 2, 7, 8, 9, 32, 33, 63, 64)
SEQ = 2**32 - 3  # + key index: crosses 2^32


def record(nb: int, kslot: int, iv12: bytes):
    seq = SEQ + kslot
    key, nonce, r, s = S.model_record(kslot, seq, iv12)
    return key, seq, nonce, S.rnd(64 * nb, f"pack model ct {nb} {kslot}"), r, s


def accumulator(r, seq, nonce, ct, **kw):
    return M.packed_accumulator(RFC7905, r, ct, seq=seq, nonce12=nonce, **kw)


@pytest.mark.parametrize("kslot", [0, 1, 2])
@pytest.mark.parametrize("nb", NBS)
def test_packed_decomposition_equals_the_reference(nb, kslot):
    key, seq, nonce, ct, r, s = record(nb, kslot, S.IVS3[12 * kslot:12 * kslot + 12])
    ad = S.tls_ad(seq, 64 * nb)
    acc = accumulator(r, seq, nonce, ct)
    assert acc == S.accumulator(key, nonce, ad, ct)
    assert ((acc + s) % (1 << 128)).to_bytes(16, "little") == R.tag_of(key, nonce, ad, ct)


@pytest.mark.parametrize("nb", [1, 33])
def test_ad_words_from_the_nonce_are_wrong_unless_the_iv_is_zero(nb):
    """The model sees the trap: with a non-zero write IV the nonce words are not the
    AD's first eight bytes; with an all-zero IV they are, and the shortcut passes."""
    for iv, same in ((S.IVS3[12:24], False), (S.IVS3[:12], False), (bytes(12), True)):
        key, seq, nonce, ct, r, _ = record(nb, 1, iv)
        want = S.accumulator(key, nonce, S.tls_ad(seq, 64 * nb), ct)
        assert accumulator(r, seq, nonce, ct) == want
        assert (accumulator(r, seq, nonce, ct, ad_from_nonce=True) == want) == same


def test_a_wrong_length_block_is_seen():
    key, seq, nonce, ct, r, _ = record(7, 0, S.IVS3[:12])
    want = S.accumulator(key, nonce, S.tls_ad(seq, 448), ct)
    draft_suffix = (448 << 40) + (1 << 104)  # the draft's last block
    assert (accumulator(r, seq, nonce, ct) - (13 + (448 << 64) + (1 << 128)) * r + draft_suffix * r) % P != want


@pytest.mark.parametrize("rbytes", [b"\xff" * 16, None], ids=["r all ones", "r drawn"])
@pytest.mark.parametrize("fill", [0xFF, 0x00, None], ids=["ct 0xff", "ct 0x00", "ct drawn"])
def test_limb_bounds_of_64_terms(rbytes, fill):
    """A 4096-byte record (64 lane terms), all-0xff ciphertext among the fills, r with
    every clamped bit set among the keys: the bounds of sg_pack.hip's header comment
    hold term by term and for the sums, and the finish gives the stream's accumulator."""
    r = int.from_bytes(rbytes or S.rnd(16, "pack bound r"), "little") & R.CLAMP
    ct = bytes([fill]) * 4096 if fill is not None else S.rnd(4096, "pack bound ct")
    M.limb_walk(RFC7905, r, ct, seq=SEQ)


def test_the_carry_bound_by_reasoning():
    """Limb 1 of a mul_add result is below 2^26 + 2^7 for every operand in bounds: the
    last column has no factor 5, so with a_i < 2^26 (a_4 < 2^27) and b_i < 2^26 + 2^8
    its carry is below 7 2^26, and 5 times that plus limb 0 carries at most 35 < 2^7."""
    b = (1 << 26) + (1 << 8)
    col4 = 4 * (1 << 26) * b + (1 << 27) * b + (1 << 32)
    assert ((col4 >> 26) * 5 + M.M26) >> 26 < 1 << 7
