"""Randomised batch parity (GPU): mixed batches drawn at random -- lengths
over every route of the device bucketing (packed 64 B-4 KiB records, the
wave-per-record buckets, the size classes, ragged and edge lengths), 16-byte
aligned or odd offsets, TLS mode (random sequence numbers, content type and
version, tls.rs:103-112) or explicit nonces and AD of a random length 0-255
(chacha20_poly1305.rs:19-42), eight keys -- sealed on the GPU and compared
byte for byte with the oracle, then opened with random tampering of the
ciphertext, the tag or (explicit mode) the AD and a few truncated records:
statuses equal the reference's Ok / Err(BadRecordMac) ("wrong mac" 1, "too
short" 2, chacha20_poly1305.rs:65-94), every other record's plaintext equals
the input, and failed records' output is zero-filled unless
SG_BATCH_KEEP_FAILED is set.
"""
from __future__ import annotations

import numpy as np
import pytest

from gpu_support import (BatchCase, check_opened, check_sealed, dev_bytes, filled, kernel_forms, open_, seal, slots,
                         tamper)

pytestmark = pytest.mark.gpu

EDGES = [0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 4032, 4095, 4096, 4097, 4160, 8192, 12352, 16320, 16383, 16384]


def _lengths(rng, count, explicit):
    kind = rng.random(count)
    lens = np.where(kind < 0.45, 64 * rng.integers(1, 257, size=count),   # packed and bucket routes
                    rng.integers(0, 16385, size=count))                    # ragged: size classes
    edges = rng.choice(EDGES, size=count)
    lens = np.where(kind > 0.9, edges, lens)
    if explicit:  # explicit mode takes records up to SG_MAX_RECORD_LEN
        big = rng.random(count) < 0.02
        lens[big] = rng.integers(16385, 32769, size=int(big.sum()))
    return lens.astype(np.uint32)


@pytest.mark.parametrize("seed", list(range(11, 27)))
def test_random_mixed_batches(gpu, oracle, seed):
    rng = np.random.default_rng(0xF022 + seed)
    count = int(rng.integers(700, 1500))
    explicit = seed % 2 == 0
    aligned = seed % 4 < 2
    lens = _lengths(rng, count, explicit)
    in_off, out_off, pt_bytes, ct_bytes = slots(lens, 16) if aligned else slots(lens, 1, (3, 7))
    pt_h = rng.bytes(pt_bytes)
    keys_h = rng.bytes(8 * 32)
    kidx = rng.integers(0, 8, size=count).astype(np.uint32)
    if explicit:
        adlen = int(rng.integers(0, 256))
        stride = max(adlen, 1)
        nonces_h = rng.bytes(8 * count)
        mode = dict(nonces_h=nonces_h, ads_h=rng.bytes(stride * count), adlen=adlen)
    else:
        seqs = rng.integers(0, 2**63, size=count, dtype=np.uint64)
        seqs[:2] = [2**32 - 1, 2**64 - 1]
        ctype, minor = int(rng.choice([20, 21, 22, 23])), int(rng.integers(0, 4))
        mode = dict(seqs=seqs, content_type=ctype, version=(3, minor))
    case = BatchCase(lens, pt_h, keys_h, in_off=in_off, out_off=out_off, kidx=kidx, **mode)

    ct_h = seal(case, filled(ct_bytes, 0))
    check_sealed(case, oracle, ct_h, where=(seed,))

    # open: tamper ~3 % of the records (ciphertext, tag or, explicit, AD), truncate a few
    flips, cut = {}, {}
    ads_in = bytearray(case.ads_h) if explicit else None
    for i in rng.choice(count, size=max(3, count // 33), replace=False):
        i, n = int(i), int(lens[i])
        where = int(rng.integers(0, 3 if explicit and adlen else 2))
        if where == 0 and n:
            flips[i] = (int(rng.integers(0, n)), 1 << int(rng.integers(0, 8)))
        elif where == 2:
            ads_in[i * stride + int(rng.integers(0, adlen))] ^= 0x20
            flips[i] = (0, 0)  # its AD instead: status 1 all the same
        else:
            flips[i] = (n + int(rng.integers(0, 16)), 0x80)
    for i in rng.choice(count, size=3, replace=False):
        cut[int(i)] = int(rng.integers(0, 16))
    exp_st, olens = tamper(case, ct_h, flips, cut)
    keep = bool(seed % 3 == 0)
    # a fresh copy of the image; 0xEE where an open writes nothing
    back_h, st_h = open_(case, dev_bytes(bytes(ct_h)), filled(pt_bytes, 0xEE), olens=olens, ads_h=ads_in,
                         keep_failed=keep)
    # nothing of a failed record is released unless kept; kept and truncated ones are not looked at
    check_opened(case, back_h, st_h, exp_st, keep=keep, where=(seed,))


@pytest.mark.parametrize("lockstep,packed", [(0, 0), (0, 1), (1, 0)])
@pytest.mark.parametrize("seed", [11, 12, 13, 14])
def test_random_mixed_batches_every_kernel_form(gpu, oracle, seed, lockstep, packed):
    """The same random batches with the wave-per-record kernel and / or the
    packed kernel switched off (sg_set_lockstep / sg_set_packed): every record
    then runs on another route (size classes), bit-exact all the same."""
    with kernel_forms(gpu, lockstep=lockstep, packed=packed):
        test_random_mixed_batches(gpu, oracle, seed)
