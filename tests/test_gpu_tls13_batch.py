"""The TLS 1.3 record batch (sg_seal_batch_tls13 / sg_open_batch_tls13) on the GPU:
the size classes over every class edge of the inner length, open of padded records,
uniform full records on the wave-per-record kernel and on the size class, tampering
on both routes, the MAC finishes on forged accumulators, and no state left behind for
the draft and RFC calls.

The reference is tests/tls13_ref.py (tied to OpenSSL by tests/test_tls13_ref.py); every
buffer is compared whole (tests/tls13_batch_support.py), so a byte written from n + 17
on fails as a wrong byte does."""
from __future__ import annotations

import functools
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import rfc8439_ref as R
import rfc_batch_support as S
import tls13_batch_support as X
import tls13_ref as T
from gpu_support import kernel_forms
from gpu_support import lockstep  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

N = X.N
COUNT = 19  # two full groups of eight and a group of three
KIDX = np.arange(COUNT, dtype=np.uint32) % 3
SEQS = (np.arange(COUNT, dtype=np.uint64) + np.uint64(2**32 - 5))
STRIDES_SEAL = (N, N + 32)        # content stride, fragment stride (n + 17 rounded up to 16)
STRIDES_OPEN = (N + 32, N + 16)   # fragment stride, inner stride

GOLD = json.loads((Path(__file__).resolve().parent / "golden" / "tls13_records.json").read_text())
# the uniform batch's key 0 and IV 0 are the golden file's, record 0 its n = 2^14, seq = 2^32 - 1 case
KEYS = bytes.fromhex(GOLD["key"]) + X.KEYS3[32:]
IVS = bytes.fromhex(GOLD["ivs"][0]) + X.IVS3[12:]
USEQS = SEQS.copy()
USEQS[0] = 2**32 - 1

# content lengths whose inner length (one more) crosses every class edge 128 << c
CLASS_LENS = (0, 1, 15, 16, 17, 47, 48, 63, 64, 65) + tuple(m - d for c in range(7) for m in [128 << c] for d in (2, 1, 0)) + (
    16383, 16384)


def rnd(n, what):
    return S.rnd(n, what)


@functools.lru_cache(maxsize=None)
def class_records():
    contents = [rnd(n, f"tls13 class {i} {n}") for i, n in enumerate(CLASS_LENS)]
    kidx = np.arange(len(contents), dtype=np.uint32) % 3
    seqs = np.arange(len(contents), dtype=np.uint64) + np.uint64(2**32 - 7)
    return contents, kidx, seqs, X.expected_sealed(contents, kidx, seqs, 22)


@functools.lru_cache(maxsize=None)
def uniform_records():
    contents = [R.data(N, b"tls13 content %d" % N)] + [rnd(N, f"tls13 uniform {i}") for i in range(1, COUNT)]
    return contents, X.expected_sealed(contents, KIDX, USEQS, 23, IVS, KEYS)


# ---------------------------------------------------------------------------
# size classes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("skew", [(0, 0), (1, 3)], ids=["aligned", "skewed"])
def test_size_classes_over_every_class_edge(gpu, skew):
    contents, kidx, seqs, want = class_records()
    frags = X.seal_whole(contents, kidx, seqs, ctype=22, skew=skew, want=want, route=0, where=("classes", skew))
    got = X.open_whole(frags, kidx, seqs, skew=skew, route=0, where=("classes", skew))
    assert got == [(T.OK, 22, n) for n in CLASS_LENS]


@pytest.mark.parametrize("skew", [(0, 0), (1, 3)], ids=["aligned", "skewed"])
def test_open_of_padded_records(gpu, skew):
    """Records as a peer may send them, built by the reference."""
    key_iv = X.key_iv
    recs = [(rnd(100, "pad c"), 23, p) for p in (1, 15, 16, 17, 255)]
    recs += [(b"", 21, 0), (b"", 22, 33), (rnd(50, "zeros c") + bytes(7), 23, 0), (rnd(50, "zeros d") + bytes(4), 23, 5),
             (rnd(N - 16, "longest"), 23, 255)]  # the last: a fragment of 2^14 + 256 bytes, the longest there is
    kidx = np.arange(len(recs) + 3, dtype=np.uint32) % 3
    seqs = np.arange(len(recs) + 3, dtype=np.uint64) + np.uint64(2**32 - 3)
    frags = [T.seal(*key_iv(int(kidx[i])), int(seqs[i]), c, t, p) for i, (c, t, p) in enumerate(recs)]
    want = [(T.OK, t, len(c)) for c, t, _ in recs]
    i = len(recs)
    frags.append(T.seal_inner(*key_iv(int(kidx[i])), int(seqs[i]), bytes(40)))      # a good tag over zeros alone
    frags.append(T.seal_inner(*key_iv(int(kidx[i + 1])), int(seqs[i + 1]), b""))    # a 16-byte fragment: the tag alone
    frags.append(T.seal(*key_iv(int(kidx[i + 2])), int(seqs[i + 2]), b"x")[:15])   # 15 bytes
    want += [(T.NO_TYPE, 0, 0), (T.NO_TYPE, 0, 0), (T.SHORT, 0, 0)]
    assert [len(f) for f in frags[-3:]] == [56, 16, 15] and len(frags[len(recs) - 1]) == T.MAX_FRAGMENT
    got = X.open_whole(frags, kidx, seqs, skew=skew, route=0, where=("padded", skew))
    assert got == want


# ---------------------------------------------------------------------------
# uniform full records: the wave-per-record kernel and the size class
# ---------------------------------------------------------------------------
def test_uniform_full_records_on_both_routes(gpu):
    contents, want = uniform_records()
    # the reference's record 0 is OpenSSL's
    g = next(c for c in GOLD["cases"] if (c["iv"], c["seq"], c["n"], c["pad"]) == (0, 2**32 - 1, N, 0))
    assert want[0][-16:].hex() == g["tag"]
    images = []
    for ls in (1, 0):
        with kernel_forms(gpu, lockstep=ls):
            frags = X.seal_whole(contents, KIDX, USEQS, strides=STRIDES_SEAL, want=want, ivs=IVS, keys=KEYS, route=ls,
                                 where=("uniform", ls))
            got = X.open_whole(frags, KIDX, USEQS, strides=STRIDES_OPEN, ivs=IVS, keys=KEYS, route=ls, where=("uniform", ls))
            assert got == [(T.OK, 23, N)] * COUNT
        images.append(frags)
    assert images[0] == images[1] == want
    assert hashlib.sha256(images[0][0][:-16]).hexdigest() == g["ct_sha256"] and images[0][0][-16:].hex() == g["tag"]


def test_full_fragment_whose_last_inner_byte_is_zero(gpu):
    """2^14 - 1 content bytes, the type and one zero of padding: the same 16401-byte
    fragment as a full record, on the same routes; the strip must walk back one byte."""
    contents = [rnd(N - 1, f"tls13 short {i}") for i in range(COUNT)]
    frags = [T.seal(*X.key_iv(int(k)), int(q), c, 23, 1) for c, k, q in zip(contents, KIDX, SEQS)]
    assert all(len(f) == N + 17 for f in frags)
    for ls in (1, 0):
        with kernel_forms(gpu, lockstep=ls):
            got = X.open_whole(frags, KIDX, SEQS, strides=STRIDES_OPEN, route=ls, where=("zero tail", ls))
        assert got == [(T.OK, 23, N - 1)] * COUNT


# ---------------------------------------------------------------------------
# tampering on both routes, clean neighbours in the same group
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ls", [1, 0])
@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper(gpu, lockstep, keep, ls):
    lockstep(ls)
    _, sealed = uniform_records()
    frags = [bytearray(f) for f in sealed]
    # content byte 0 and 2^14 - 1, the tail byte, the tag's first and last byte
    flips = {1: (0, 0x01), 4: (N - 1, 0x80), 9: (N, 0x10), 12: (N + 1, 0x01), 16: (N + 16, 0x80)}
    for i, (at, mask) in flips.items():
        frags[i][at] ^= mask
    seqs = USEQS.copy()
    seqs[17] ^= np.uint64(1)  # a wrong sequence number
    bad = set(flips) | {17}
    got = X.open_whole([bytes(f) for f in frags], KIDX, seqs, strides=STRIDES_OPEN, keep=keep, ivs=IVS, keys=KEYS, route=ls,
                       where=("tamper", ls, keep))
    assert got == [(T.BAD_MAC, 0, 0) if i in bad else (T.OK, 23, N) for i in range(COUNT)]
    # a wrong first IV word of key 1: its records fail, their neighbours do not
    ivs = bytearray(IVS)
    ivs[12] ^= 0x40
    got = X.open_whole(sealed, KIDX, USEQS, strides=STRIDES_OPEN, keep=keep, ivs=bytes(ivs), keys=KEYS, route=ls,
                       where=("tamper iv", ls, keep))
    assert got == [(T.BAD_MAC, 0, 0) if i % 3 == 1 else (T.OK, 23, N) for i in range(COUNT)]


@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper_in_the_size_classes(gpu, keep):
    """The listed batch: a flip in the content, in the type byte and in the tag of small records."""
    contents, kidx, seqs, sealed = class_records()
    frags = [bytearray(f) for f in sealed]
    idx = {n: i for i, n in enumerate(CLASS_LENS)}
    flips = {idx[64]: (0, 0x01), idx[65]: (65, 0x04), idx[127]: (128, 0x80), idx[0]: (0, 0x01), idx[16384]: (N + 16, 0x01)}
    for i, (at, mask) in flips.items():
        frags[i][at] ^= mask
    got = X.open_whole([bytes(f) for f in frags], kidx, seqs, skew=(1, 3), keep=keep, where=("tamper classes", keep))
    assert got == [(T.BAD_MAC, 0, 0) if i in flips else (T.OK, 22, n) for i, n in enumerate(CLASS_LENS)]


# ---------------------------------------------------------------------------
# the MAC finishes on forged accumulators
# ---------------------------------------------------------------------------
def ff_record(n: int, k: int, seq0: int):
    """(content, type, seq) whose sealed inner ciphertext is n + 1 bytes of 0xff."""
    for seq in range(seq0, seq0 + 16):
        key, iv = X.key_iv(k)
        pt = R.xor_stream(key, T.nonce(iv, seq), b"\xff" * (n + 1))
        if pt[n]:
            return pt[:n], pt[n], seq
    raise AssertionError("no non-zero type in 16 sequence numbers")


def test_wpr_finish_on_forged_accumulators(gpu):
    """Full records (AD 5 bytes, n = 2^14 + 1) whose accumulator before the final reduction
    is == 0, p - 1, p, p + 4 and 2^130 - 1 (mod p), and one whose ciphertext is all 0xff."""
    names = list(S.ACC_TARGETS)
    kidx = np.zeros(len(names), dtype=np.uint32)
    seqs = np.arange(len(names), dtype=np.uint64) + np.uint64(7)
    contents = [X.forge_content(0, int(seqs[i]), N, S.ACC_TARGETS[k], f"wpr {k}") for i, k in enumerate(names)]
    want = X.expected_sealed(contents, kidx, seqs)
    ff, ff_type, ff_seq = ff_record(N, 1, 100)
    for ls in (1, 0):
        with kernel_forms(gpu, lockstep=ls):
            frags = X.seal_whole(contents, kidx, seqs, strides=STRIDES_SEAL, want=want, route=ls, where=("forged wpr", ls))
            assert X.open_whole(frags, kidx, seqs, strides=STRIDES_OPEN, route=ls) == [(T.OK, 23, N)] * len(names)
            f = X.seal_whole([ff], [1], [ff_seq], ctype=ff_type, strides=STRIDES_SEAL, route=ls, where=("0xff wpr", ls))
            assert f[0][:-16] == b"\xff" * (N + 1)
            assert X.open_whole(f, [1], [ff_seq], strides=STRIDES_OPEN, route=ls) == [(T.OK, ff_type, N)]


def test_class_finish_on_forged_accumulators(gpu):
    """The same for the size-class finish: 64 content bytes, n = 65."""
    names = list(S.ACC_TARGETS)
    kidx = np.arange(len(names), dtype=np.uint32) % 3
    seqs = np.arange(len(names), dtype=np.uint64) + np.uint64(2**32 - 2)
    contents = [X.forge_content(int(kidx[i]), int(seqs[i]), 64, S.ACC_TARGETS[k], f"class {k}") for i, k in enumerate(names)]
    frags = X.seal_whole(contents, kidx, seqs, where=("forged class",))
    assert X.open_whole(frags, kidx, seqs) == [(T.OK, 23, 64)] * len(names)
    ff, ff_type, ff_seq = ff_record(64, 2, 200)
    f = X.seal_whole([ff], [2], [ff_seq], ctype=ff_type, where=("0xff class",))
    assert f[0][:-16] == b"\xff" * 65
    assert X.open_whole(f, [2], [ff_seq]) == [(T.OK, ff_type, 64)]


# ---------------------------------------------------------------------------
# no state left behind
# ---------------------------------------------------------------------------
def test_draft_and_rfc_calls_around_a_tls13_call(gpu, oracle):
    """A draft call and an RFC 7905 call before and after a TLS 1.3 call, all on the cached
    workspace: both give their known outputs, and so does the TLS 1.3 call between them."""
    import torch

    from gpu_support import BatchCase, check_opened, check_sealed, open_, seal, slots, uninit

    def draft():
        lens = np.array([0, 1, 64, 100, 4096, N], dtype=np.uint32)
        in_off, out_off, pt_bytes, ct_bytes = slots(lens, 16)
        case = BatchCase(lens, rnd(pt_bytes, "leak draft"), in_off=in_off, out_off=out_off, seq0=2**32 - 2)
        out = uninit(ct_bytes)
        sealed = seal(case, out)
        check_sealed(case, oracle, sealed, where=("draft",))
        back, st = open_(case, out, uninit(pt_bytes))
        check_opened(case, back, st, bytes(case.count), keep=False, where=("draft",))

    def rfc():
        case = S.listed_case((0, 1, 64, 100, 4096, N), mode="tls", kidx=np.arange(6, dtype=np.uint32) % 3, ivs_h=S.IVS3,
                             seq0=2**32 - 2, tag="leak rfc")
        S.open_whole(case, S.seal_whole(case), bytes(case.count))
        ucase = S.uniform_case(N, 9, mode="tls", kidx=np.arange(9, dtype=np.uint32) % 3, ivs_h=S.IVS3, seq0=5, tag="leak urfc")
        S.open_whole(ucase, S.seal_whole(ucase), bytes(ucase.count))

    def tls13():
        contents, want = uniform_records()
        frags = X.seal_whole(contents[:9], KIDX[:9], USEQS[:9], strides=STRIDES_SEAL, want=want[:9], ivs=IVS, keys=KEYS, route=1)
        assert X.open_whole(frags, KIDX[:9], USEQS[:9], strides=STRIDES_OPEN, ivs=IVS, keys=KEYS, route=1) == [(T.OK, 23, N)] * 9
        c, kidx, seqs, w = class_records()
        assert X.open_whole(X.seal_whole(c, kidx, seqs, ctype=22, want=w), kidx, seqs) == [(T.OK, 22, n) for n in CLASS_LENS]

    for call in (draft, rfc, tls13, draft, rfc, tls13):
        call()
    torch.cuda.synchronize()
