"""The RFC 8439 record batch on uniform 16 KiB records: the wave-per-record kernel
(lockstep on) and the size class (lockstep off) must both give the reference's
bytes, and so each other's; a mixed TLS batch must give the same bytes under every
setting of the kernel-form switches; the wave-per-record finish on forged
accumulators.

The reference is tests/rfc8439_ref.py; every buffer is compared whole
(tests/rfc_batch_support.py)."""
from __future__ import annotations

import numpy as np
import pytest

import rfc8439_ref as R
import rfc_batch_support as S
from gpu_support import kernel_forms, tamper
from gpu_support import lockstep, packed  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

N = 16384
COUNT = 19  # two full groups of eight and a partial one
KIDX = np.arange(COUNT, dtype=np.uint32) % 3


def both_settings(gpu, case, where):
    """Seal and open under lockstep 1 and 0; the two sealed images are equal."""
    images = []
    for ls in (1, 0):
        with kernel_forms(gpu, lockstep=ls):
            sealed = S.seal_whole(case, where=(*where, "lockstep", ls))
            S.open_whole(case, sealed, bytes(case.count), where=(*where, "lockstep", ls))
        images.append(sealed)
    assert images[0] == images[1], (*where, "the two lockstep settings differ")
    return images[0]


def test_tls_mode_seq_edges(gpu):
    seqs = np.array([(S.SEQ_EDGES[i % len(S.SEQ_EDGES)] + 3 * (i // len(S.SEQ_EDGES))) % 2**64 for i in range(COUNT)], dtype=np.uint64)
    case = S.uniform_case(N, COUNT, mode="tls", kidx=KIDX, ivs_h=S.IVS3, seqs=seqs, content_type=22, version=(3, 1),
                          tag="wpr tls")
    both_settings(gpu, case, ("tls seqs",))


def test_tls_mode_seq0_across_2_32(gpu):
    case = S.uniform_case(N, COUNT, mode="tls", kidx=KIDX, ivs_h=S.IVS3, seq0=2**32 - 9, tag="wpr seq0")
    both_settings(gpu, case, ("tls seq0",))


@pytest.mark.parametrize("adlen", [0, 5, 13, 15, 16, 17, 255])
def test_explicit_mode(gpu, adlen):
    case = S.uniform_case(N, COUNT, mode=adlen, kidx=KIDX, tag=f"wpr x{adlen}")
    both_settings(gpu, case, ("explicit", adlen))


@pytest.mark.parametrize("ls", [1, 0])
@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper(gpu, lockstep, keep, ls):
    """A bit in chunk 0, in chunk 3 and in the tag; untampered records beside them."""
    lockstep(ls)
    seqs = np.arange(COUNT, dtype=np.uint64) + np.uint64(2**32 - 5)
    case = S.uniform_case(N, COUNT, mode="tls", kidx=KIDX, ivs_h=S.IVS3, seqs=seqs, tag="wpr tamper")
    sealed = bytearray(S.seal_whole(case))
    flips = {1: (0, 0x01), 4: (4095, 0x80), 9: (3 * 4096 + 7, 0x10), 12: (N - 1, 0x80), 16: (N, 0x01), 17: (N + 8, 0x40),
             18: (N + 15, 0x80)}
    exp_st, _ = tamper(case, sealed, flips)
    S.open_whole(case, bytes(sealed), exp_st, keep=keep, where=("tamper", ls, keep))


# ---------------------------------------------------------------------------
# a mixed TLS batch: the switches cannot misroute RFC records
# ---------------------------------------------------------------------------
MIXED = tuple(range(64, N + 1, 64)) + (0, 1, 63, 65, 100, 4097, 16383, 16385)


def test_mixed_tls_batch_under_every_switch_setting(gpu):
    """In the draft these lengths go to the packed kernel and the J = 2..4 buckets; in
    RFC form they stay on the size classes, whatever the switches say."""
    kidx = np.arange(len(MIXED), dtype=np.uint32) % 3
    case = S.listed_case(MIXED, mode="tls", kidx=kidx, ivs_h=S.IVS3, seq0=2**32 - 100, tag="mixed")
    images = []
    for ls in (1, 0):
        for pk in (1, 0):
            with kernel_forms(gpu, lockstep=ls, packed=pk):
                sealed = S.seal_whole(case, where=("mixed", ls, pk))
                if ls == pk:
                    S.open_whole(case, sealed, bytes(case.count), where=("mixed", ls, pk))
            images.append(sealed)
    assert all(im == images[0] for im in images)


# ---------------------------------------------------------------------------
# the wave-per-record finish on forged accumulators
# ---------------------------------------------------------------------------
def test_wpr_finish_on_forged_accumulators(gpu):
    """16 KiB records whose accumulator before the final reduction is == 0, p - 1, p,
    p + 4 and 2^130 - 1 (mod p), through both lockstep settings."""
    ad_len = 13
    names = list(S.ACC_TARGETS)
    key = S.KEYS3[:32]
    nonces = [S.rnd(12, f"wpr forge nonce {k}") for k in names]
    ads = [S.rnd(ad_len, f"forge ad {i}") for i in range(len(names))]
    pts = []
    for i, k in enumerate(names):
        ct, tries = S.forge_ct(key, nonces[i], ads[i], N, S.ACC_TARGETS[k], f"wpr {k}")
        assert tries <= 200 and S.accumulator(key, nonces[i], ads[i], ct) == S.ACC_TARGETS[k] % S.P
        pts.append(R.xor_stream(key, nonces[i], ct))
    case = S.uniform_case(N, len(names), mode=ad_len, keys=key, pts=pts, nonces=b"".join(nonces), ads=ads)
    both_settings(gpu, case, ("forged", "wpr"))
