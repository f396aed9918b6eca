"""CPU check of the packed kernel's Poly1305 in TLS 1.3 form
(sg_pack_kernel<OPEN, Construction::kRfc8439, true>, suruga_amd/csrc/sg_pack.hip) with the
model of tests/pack_model.py, form TLS13.

A TLS 1.3 record whose inner plaintext is n = 64 nb bytes has the MAC stream
AD(5) || 0^11 || ct || le64(5) || le64(n), B = 4 nb + 2 full blocks, the AD the record
header 17 03 03 be16(n + 16).  Lane terms, weights and tables are the RFC form's
(tests/test_pack_mac_model_rfc8439.py); block0 is built from n alone.  The tag must be
the reference's for tests/tls13_ref.py's header, and the limb bounds that sg_pack.hip's
header comment derives for the RFC stream must hold for this one along
pack_model.limb_walk, all-0xff ciphertext included."""
from __future__ import annotations

import pytest

import pack_model as M
import rfc8439_ref as R
import rfc_batch_support as S
import tls13_ref as T
from pack_model import RFC7905, TLS13

P = M.P
NBS = (1, 2, 33, 64)
SEQ = 2**32 - 3


def record(nb: int, kslot: int, fill):
    key, nonce, r, s = S.model_record(kslot, SEQ + kslot)
    assert nonce == T.nonce(S.IVS3[12 * kslot:12 * kslot + 12], SEQ + kslot)
    ct = bytes([fill]) * (64 * nb) if fill is not None else S.rnd(64 * nb, f"pack13 model ct {nb} {kslot}")
    return key, nonce, ct, r, s


def test_block0_is_the_record_header():
    for n in (64, 192, 240, 4096):
        w = M.block0_words(TLS13, n)
        assert b"".join(x.to_bytes(4, "little") for x in w) == T.header(n + 16) + bytes(11)


@pytest.mark.parametrize("fill", [None, 0xFF], ids=["ct drawn", "ct 0xff"])
@pytest.mark.parametrize("kslot", [0, 1, 2])
@pytest.mark.parametrize("nb", NBS)
def test_packed_decomposition_equals_the_reference(nb, kslot, fill):
    key, nonce, ct, r, s = record(nb, kslot, fill)
    ad = T.header(64 * nb + 16)
    acc = M.packed_accumulator(TLS13, r, ct)
    assert acc == S.accumulator(key, nonce, ad, ct)
    assert ((acc + s) % (1 << 128)).to_bytes(16, "little") == R.tag_of(key, nonce, ad, ct)


def test_the_rfc7905_constant_term_is_seen():
    """The 13-byte AD's constant term (or its length block alone) gives another accumulator."""
    key, nonce, ct, r, _ = record(7, 0, None)
    want = S.accumulator(key, nonce, T.header(448 + 16), ct)
    assert M.packed_accumulator(TLS13, r, ct) == want
    assert M.packed_accumulator(RFC7905, r, ct, seq=SEQ, nonce12=nonce) != want
    assert (M.packed_accumulator(TLS13, r, ct) + (13 - 5) * r) % P != want


@pytest.mark.parametrize("nb", NBS)
@pytest.mark.parametrize("rbytes", [b"\xff" * 16, None], ids=["r all ones", "r drawn"])
@pytest.mark.parametrize("fill", [0xFF, None], ids=["ct 0xff", "ct drawn"])
def test_limb_bounds_along_the_kernel_arithmetic(nb, rbytes, fill):
    """The kernel's words, step by step: every bound of sg_pack.hip's header comment is
    asserted on the way, and the finish with this stream's constant term gives its accumulator."""
    r = int.from_bytes(rbytes or S.rnd(16, "pack13 bound r"), "little") & R.CLAMP
    ct = bytes([fill]) * (64 * nb) if fill is not None else S.rnd(64 * nb, f"pack13 bound ct {nb}")
    M.limb_walk(TLS13, r, ct)
