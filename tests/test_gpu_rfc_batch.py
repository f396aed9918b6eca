"""The RFC 8439 record batch (sg_seal_batch_rfc8439 / sg_open_batch_rfc8439) on the
size classes: explicit 12-byte nonces and the RFC 7905 TLS mode, listed and uniform
batches, tampering, the scrub, and the draft calls untouched beside it.

The reference is tests/rfc8439_ref.py (tied to OpenSSL).  Every device buffer starts
as a sentinel with margins and is compared whole (tests/rfc_batch_support.py), so a
stray write fails too; every record of every batch is compared."""
from __future__ import annotations

import numpy as np
import pytest

import rfc8439_ref as R
import rfc_batch_support as S
from gpu_support import BatchCase, check_sealed, filled, tamper
from gpu_support import lockstep, packed  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 18432, 32768)
ADLENS = (0, 1, 5, 12, 13, 15, 16, 17, 31, 32, 255)
KIDX = np.array([i % 3 for i in range(len(LENGTHS))], dtype=np.uint32)


@pytest.mark.parametrize("skew", [(0, 0), (1, 3)], ids=["aligned", "skew13"])
@pytest.mark.parametrize("adlen", ADLENS)
def test_size_classes_explicit_mode(gpu, adlen, skew):
    """Every length edge of every size class in one listed batch, three keys by key_index."""
    case = S.listed_case(LENGTHS, mode=adlen, skew=skew, kidx=KIDX, tag=f"x{adlen}")
    sealed = S.seal_whole(case, where=("explicit", adlen, skew))
    S.open_whole(case, sealed, bytes(case.count), where=("explicit", adlen, skew))


@pytest.mark.parametrize("skew", [(0, 0), (1, 3)], ids=["aligned", "skew13"])
def test_size_classes_tls_mode(gpu, skew):
    """RFC 7905: three keys with three IVs (one all 0xFF), the sequence-number edges, a
    non-default content type and version."""
    lens = LENGTHS  # all <= 65535
    seqs = np.array([(S.SEQ_EDGES[i % len(S.SEQ_EDGES)] + 3 * (i // len(S.SEQ_EDGES))) % 2**64 for i in range(len(lens))],
                    dtype=np.uint64)
    case = S.listed_case(lens, mode="tls", skew=skew, kidx=KIDX, ivs_h=S.IVS3, seqs=seqs, content_type=22,
                         version=(3, 1), tag="tls")
    sealed = S.seal_whole(case, where=("tls", skew))
    S.open_whole(case, sealed, bytes(case.count), where=("tls", skew))


def test_tls_mode_default_header_and_seq0(gpu):
    """seq0 + i across 2^32 with the default header (application_data, 3.3)."""
    lens = (100, 0, 4096, 17, 1024)
    case = S.listed_case(lens, mode="tls", kidx=KIDX[:5], ivs_h=S.IVS3, seq0=2**32 - 2, tag="seq0")
    sealed = S.seal_whole(case)
    S.open_whole(case, sealed, bytes(case.count))


@pytest.mark.parametrize("mode", ["tls", 13])
@pytest.mark.parametrize("n", [64, 4096, 16400])
def test_uniform_strided_through_the_class_route(gpu, lockstep, n, mode):
    """Uniform batches that the wave-per-record kernel does not take."""
    lockstep(0)
    count = 9
    kw = dict(ivs_h=S.IVS3, seq0=2**32 - 4) if mode == "tls" else {}
    case = S.uniform_case(n, count, mode=mode, kidx=np.arange(count, dtype=np.uint32) % 3, tag=f"u{n}", **kw)
    sealed = S.seal_whole(case, where=(n, mode))
    S.open_whole(case, sealed, bytes(count), where=(n, mode))


# ---------------------------------------------------------------------------
# tampering and the scrub
# ---------------------------------------------------------------------------
T_LENS = (100, 100, 100, 100, 100, 100, 4097, 20, 1024, 64, 333, 100)


@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper_explicit(gpu, keep):
    """One bit in the first and the last ct byte and in each tag word; a record cut
    below a tag; untampered records between them.  The scrub zeroes exactly n bytes."""
    case = S.listed_case(T_LENS, mode=13, kidx=np.arange(len(T_LENS), dtype=np.uint32) % 3, tag="tamper")
    sealed = bytearray(S.seal_whole(case))
    flips = {0: (0, 0x01), 1: (99, 0x80), 2: (100, 0x01), 3: (104, 0x10), 4: (108, 0x02), 5: (115, 0x80),
             6: (4096, 0x04), 8: (1024 + 15, 0x80)}
    exp_st, olens = tamper(case, sealed, flips, truncate={7: 15})
    S.open_whole(case, bytes(sealed), exp_st, keep=keep, olens=olens, where=("tamper", keep))


@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_padding_forgery_fails(gpu, keep):
    """ad || 00 pads to the same 16 bytes as ad: only the length block tells them apart.
    The same ct and tag opened with one more zero AD byte must fail, for every record."""
    lens = (0, 1, 16, 100, 4096)
    case = S.listed_case(lens, mode=13, tag="padforge")
    sealed = S.seal_whole(case)
    longer = S.RfcCase(case.lens, case.pt_h, case.keys_h, in_off=case.in_off, out_off=case.out_off,
                       nonces_h=case.nonces_h, ads_h=b"".join(case.ads_h[13 * i:13 * i + 13] + b"\0" for i in range(5)),
                       adlen=14)
    S.open_whole(longer, sealed, b"\1" * 5, keep=keep, where=("padding forgery", keep))
    S.open_whole(case, sealed, bytes(5), keep=keep)


@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper_tls_wrong_seq_and_wrong_iv(gpu, keep):
    lens = (100, 1024, 4097, 16, 0, 64)
    seqs = np.array([5, 2**32 - 1, 2**32, 7, 8, 2**64 - 1], dtype=np.uint64)
    kidx = np.array([0, 1, 2, 0, 1, 2], dtype=np.uint32)
    case = S.listed_case(lens, mode="tls", kidx=kidx, ivs_h=S.IVS3, seqs=seqs, tag="tlst")
    sealed = S.seal_whole(case)
    # a wrong sequence number for records 1 and 5: another nonce and another AD
    wrong = seqs.copy()
    wrong[1] += 1
    wrong[5] -= 1
    other = S.listed_case(lens, mode="tls", kidx=kidx, ivs_h=S.IVS3, seqs=wrong, tag="tlst")
    S.open_whole(other, sealed, bytes([0, 1, 0, 0, 0, 1]), keep=keep, where=("wrong seq", keep))
    # a wrong IV for key 1 (one bit in its last byte): records 1 and 4 fail
    bad_iv = bytearray(S.IVS3)
    bad_iv[12 + 11] ^= 0x01
    other = S.listed_case(lens, mode="tls", kidx=kidx, ivs_h=bytes(bad_iv), seqs=seqs, tag="tlst")
    S.open_whole(other, sealed, bytes([0, 1, 0, 0, 1, 0]), keep=keep, where=("wrong iv", keep))
    # ... and one bit in its first word (state word 13)
    bad_iv = bytearray(S.IVS3)
    bad_iv[24] ^= 0x80
    other = S.listed_case(lens, mode="tls", kidx=kidx, ivs_h=bytes(bad_iv), seqs=seqs, tag="tlst")
    S.open_whole(other, sealed, bytes([0, 0, 1, 0, 0, 1]), keep=keep, where=("wrong iv word 13", keep))


# ---------------------------------------------------------------------------
# the draft beside it
# ---------------------------------------------------------------------------
def test_draft_calls_untouched_by_an_rfc_call_between_them(gpu, oracle):
    """Draft, RFC, draft in one process: both draft outputs are the oracle's, and equal."""
    from gpu_support import seal, slots

    lens = np.array([0, 17, 100, 1024, 4096, 5000])
    in_off, out_off, pt_bytes, ct_bytes = slots(lens, 16)
    pt = S.rnd(pt_bytes, "draft between")
    draft = BatchCase(lens, pt, in_off=in_off, out_off=out_off, seq0=2**32 - 3)
    outs = []
    for leg in range(2):
        out = filled(ct_bytes, 0)
        outs.append(bytes(seal(draft, out)))
        check_sealed(draft, oracle, outs[-1], where=("draft leg", leg))
        if leg == 0:
            rfc = S.listed_case(lens, mode="tls", ivs_h=S.IVS3[:12], keys=draft.keys_h, seq0=2**32 - 3, tag="between")
            S.seal_whole(rfc, where=("rfc between",))
    assert outs[0] == outs[1] == bytes(draft.sealed_image(oracle, ct_bytes))


# ---------------------------------------------------------------------------
# the Poly1305 finish of the class kernel on forged accumulators
# ---------------------------------------------------------------------------
def test_class_finish_on_forged_accumulators(gpu, lockstep):
    """Records of 4096 bytes whose accumulator before the final reduction is == 0, p - 1,
    p, p + 4 and 2^130 - 1 (mod p): tags against the reference."""
    lockstep(1)
    n, ad_len = 4096, 13
    names = list(S.ACC_TARGETS)
    nonces = [S.rnd(12, f"class forge nonce {k}") for k in names]
    ads = [S.rnd(ad_len, f"forge ad {i}") for i in range(len(names))]
    pts = []
    for i, k in enumerate(names):
        ct, tries = S.forge_ct(S.KEYS3[:32], nonces[i], ads[i], n, S.ACC_TARGETS[k], f"class {k}")
        assert tries <= 200 and S.accumulator(S.KEYS3[:32], nonces[i], ads[i], ct) == S.ACC_TARGETS[k] % S.P
        pts.append(R.xor_stream(S.KEYS3[:32], nonces[i], ct))
    case = S.uniform_case(n, len(names), mode=ad_len, keys=S.KEYS3[:32], pts=pts, nonces=b"".join(nonces), ads=ads)
    sealed = S.seal_whole(case, where=("forged", "class"))
    S.open_whole(case, sealed, bytes(len(names)), where=("forged", "class"))
