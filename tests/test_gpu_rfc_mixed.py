"""Mixed TLS batches through sg_*_batch_rfc8439 on the routed kernels: the packed
kernel (64 B-4 KiB) and the J = 2..4 wave-per-record buckets in RFC 8439 / RFC 7905
form, beside the size classes.

The reference is tests/rfc8439_ref.py; every buffer is a sentinel buffer compared
whole (tests/rfc_batch_support.py).  Every batch is a listed TLS batch over the three
keys KEYS3 with the write IVs IVS3 (one of them all 0xff) and seq0 = 2^32 - 100, so
that the sequence numbers cross 2^32.  Which kernel took a record is read from
sg_last_batch_routes and held against the route predicates of tests/footprint.py."""
from __future__ import annotations

import numpy as np
import pytest

import footprint as fp
import rfc8439_ref as R
import rfc_batch_support as S
from gpu_support import BatchCase, dev_u8, host_np, kernel_forms, slots, tamper

pytestmark = pytest.mark.gpu

SEQ0 = 2**32 - 100
NB_CYCLE = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64)
INELIGIBLE = (0, 1, 63, 65, 100, 4097)
BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)
M = S.M


def kidx_of(count: int) -> np.ndarray:
    return np.arange(count, dtype=np.uint32) % 3


def rfc_case(lens, tag: str, **kw) -> S.RfcCase:
    return S.listed_case(lens, mode="tls", kidx=kidx_of(len(lens)), ivs_h=S.IVS3, seq0=SEQ0, tag=tag, **kw)


def packed_edge_lens():
    """257 packed records (two full runs of 128 and a run of one) with the ineligible
    lengths spread among them."""
    lens = [64 * NB_CYCLE[i % len(NB_CYCLE)] for i in range(257)]
    for k, n in enumerate(INELIGIBLE):
        lens.insert(40 * k + 3, n)
    return lens


def bucket_edge_lens():
    """19 records of every bucket length, interleaved so that a group of eight holds
    different lengths, and a few small records."""
    lens = [BUCKET_NS[i % len(BUCKET_NS)] for i in range(19 * len(BUCKET_NS))]
    for k, n in enumerate((64, 100, 0, 640)):
        lens.insert(30 * k + 1, n)
    return lens


def model_routes(case: BatchCase, open_: bool, lockstep: bool = True, packed: bool = True) -> dict:
    """What sg_last_batch_routes must say, from tests/footprint.py's predicates (every
    device buffer of this file starts 16-byte aligned; the offsets are the addresses)."""
    ns = [int(n) for n in case.lens]
    src, dst = (case.out_off, case.in_off) if open_ else (case.in_off, case.out_off)
    buckets, pk = fp.mixed_routes(max(ns), True, True, lockstep, packed)
    counts = fp.route_counts(ns, src, dst, buckets, pk)
    return {"known": True, "classes": sum(v for k, v in counts.items() if k[0] == "class"),
            "bucket": [counts.get(("bucket", J), 0) for J in (2, 3, 4)], "packed": counts.get(("packed",), 0),
            "skipped": 0}


def last_routes() -> dict:
    from suruga_amd import batch as B

    return B.last_routes()


def seal_open(case: S.RfcCase, where, lockstep=True, packed=True) -> bytes:
    sealed = S.seal_whole(case, where=where)
    assert last_routes() == model_routes(case, False, lockstep, packed), (*where, "seal routes")
    S.open_whole(case, sealed, bytes(case.count), where=where)
    assert last_routes() == model_routes(case, True, lockstep, packed), (*where, "open routes")
    return sealed


@pytest.fixture(scope="module")
def packed_case():
    return rfc_case(packed_edge_lens(), "mixed packed")


@pytest.fixture(scope="module")
def bucket_case():
    return rfc_case(bucket_edge_lens(), "mixed bucket")


# ---------------------------------------------------------------------------
# 1, 2: the edges of each route
# ---------------------------------------------------------------------------
def test_packed_edges(gpu, packed_case):
    """Chunk-straddling records, both table-index boundaries (nb = 8, 9 and 32, 33),
    more than eight chunks per run, a partial last round and a run of one record."""
    case = packed_case
    assert int(case.lens.sum()) < 500_000
    seal_open(case, ("packed edges",))
    r = last_routes()
    assert r["packed"] == 257 and r["classes"] == len(INELIGIBLE) and r["bucket"] == [0, 0, 0]


def test_bucket_edges(gpu, bucket_case):
    """Every bucket's shortest and longest record, two full groups of eight and a
    partial one per bucket."""
    case = bucket_case
    seal_open(case, ("bucket edges",))
    r = last_routes()
    assert r["bucket"] == [38, 38, 57] and r["packed"] == 2 and r["classes"] == 2


# ---------------------------------------------------------------------------
# 3: the routes give the same bytes, and the diagnostic says which ran
# ---------------------------------------------------------------------------
def draft_twin(case: S.RfcCase) -> BatchCase:
    return BatchCase(case.lens, case.pt_h, case.keys_h, in_off=case.in_off, out_off=case.out_off, kidx=case.kidx,
                     seq0=case.seq0)


def draft_seal_whole(case: BatchCase, oracle, where=()) -> bytes:
    """S.seal_whole for a draft batch: the whole sentinel buffer against the oracle's bytes."""
    import torch

    from suruga_amd import batch as B

    size = M + fp.round_up(max(case.out_range(i)[1] for i in range(case.count)), 16) + M
    want = fp.image(size, 0x6B, [(M + int(case.out_off[i]), case.expected(oracle, i)) for i in range(case.count)])
    d_in = dev_u8(np.concatenate([fp.sentinel(M, 0x35), np.frombuffer(case.pt_h, dtype=np.uint8), fp.sentinel(M, 0x36)]))
    d_out = dev_u8(fp.sentinel(size, 0x6B))
    B.seal(B.Batch(inp=d_in[M:], out=d_out[M:], **case.seal_args()))
    torch.cuda.synchronize()
    got = host_np(d_out)
    rs = [(M + lo, M + hi) for lo, hi in (case.out_range(i) for i in range(case.count))]
    assert (d := fp.first_diff(got, want, rs)) is None, (*where, "draft seal output", d)
    return got[M:size - M].tobytes()


@pytest.mark.parametrize("which", ["packed", "bucket"])
def test_route_equality_and_the_diagnostic(gpu, oracle, packed_case, bucket_case, which):
    case = packed_case if which == "packed" else bucket_case
    images = {}
    for ls in (1, 0):
        for pk in (1, 0):
            with kernel_forms(gpu, lockstep=ls, packed=pk):
                images[ls, pk] = S.seal_whole(case, where=(which, ls, pk))
                got = last_routes()
            assert got == model_routes(case, False, bool(ls), bool(pk)), (which, ls, pk)
            if (ls, pk) == (0, 0):
                assert got["known"] and got["packed"] == 0 and got["bucket"] == [0, 0, 0]
                assert got["classes"] == case.count
            if (ls, pk) == (1, 1):  # an RFC call takes the routed kernels
                assert got["packed"] > 0
                if which == "bucket":
                    assert sum(got["bucket"]) > 0
    assert all(im == images[1, 1] for im in images.values()), which
    # a draft call of the same lengths: the same populations, the predicates' own
    draft = draft_twin(case)
    with kernel_forms(gpu, lockstep=1, packed=1):
        draft_seal_whole(draft, oracle, where=(which, "draft"))
        got = last_routes()
    assert got == model_routes(draft, False)
    assert got["packed"] > 0 and (which == "packed" or sum(got["bucket"]) > 0)


# ---------------------------------------------------------------------------
# 4: open
# ---------------------------------------------------------------------------
TAMPER_CLASS_NS = (65, 100, 1000, 4097, 200, 3000, 16383, 127)
TAMPER_PACKED_NS = (64, 128, 4096, 2048, 64, 576, 1024, 4032, 64, 512)
SHORT_NS = (40, 64)


def tamper_lens():
    """Eight records or more on every route, the routes interleaved; two records that
    the open cuts below a tag's length."""
    cols = [TAMPER_PACKED_NS, TAMPER_CLASS_NS, (4160, 8192) * 4, (8256, 12288) * 4, (12352, 16320, 16384, 16384) * 2]
    lens = [c[i] for i in range(10) for c in cols if i < len(c)]
    return lens + list(SHORT_NS)


@pytest.fixture(scope="module")
def tamper_case():
    return rfc_case(tamper_lens(), "mixed tamper")


def route_members(case: BatchCase) -> dict:
    """Record indices by route (open direction), the short records left out."""
    out: dict = {}
    for i in range(case.count - len(SHORT_NS)):
        key = fp.route(case.n(i), int(case.out_off[i]), int(case.in_off[i]), True, True)
        out.setdefault(key if key[0] != "class" else ("class",), []).append(i)
    return out


@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper_on_every_route(gpu, tamper_case, keep):
    """A bit in the first block, in the last block and in three tag bytes of records on
    each route, untampered records between them in the same run and group; two records
    shorter than a tag in the same call."""
    case = tamper_case
    members = route_members(case)
    assert sorted(members) == [("bucket", 2), ("bucket", 3), ("bucket", 4), ("class",), ("packed",)]
    flips = {}
    for rs in members.values():
        assert len(rs) >= 8
        n = case.n
        flips.update({rs[1]: (0, 0x01), rs[3]: (n(rs[3]) - 1, 0x80), rs[4]: (n(rs[4]), 0x01),
                      rs[6]: (n(rs[6]) + 8, 0x40), rs[7]: (n(rs[7]) + 15, 0x80)})
    sealed = bytearray(S.seal_whole(case))
    truncate = {case.count - 2: 7, case.count - 1: 15}
    exp_st, olens = tamper(case, sealed, flips, truncate)
    assert exp_st.count(1) == 25 and exp_st.count(2) == 2
    S.open_whole(case, bytes(sealed), exp_st, keep=keep, olens=olens, where=("tamper", keep))
    r = last_routes()
    assert r["known"] and r["packed"] == len(members["packed",]) and \
        r["bucket"] == [len(members["bucket", J]) for J in (2, 3, 4)]


def test_a_wrong_iv_table_fails_every_record(gpu, tamper_case):
    """One bit of every IV's first word (state word 13 alone): no route may ignore it."""
    case = tamper_case
    sealed = S.seal_whole(case)
    wrong = bytearray(S.IVS3)
    for k in range(3):
        wrong[12 * k] ^= 0x04
    _, olens = tamper(case, bytearray(sealed), None, {case.count - 2: 7, case.count - 1: 15})
    exp_st = bytes([1] * (case.count - 2) + [2, 2])
    S.open_whole(case, sealed, exp_st, olens=olens, ivs_h=bytes(wrong), where=("wrong ivs",))
    assert last_routes()["packed"] == len(route_members(case)["packed",])


# ---------------------------------------------------------------------------
# 5: the finish of each route on forged accumulators
# ---------------------------------------------------------------------------
FORGE_NS = (64, 4096, 8192, 12288, 16384)


def test_finish_edges_on_forged_accumulators(gpu):
    """Records whose accumulator before the final reduction is == 0, p - 1, p, p + 4 and
    2^130 - 1 (mod p): on the packed finish n = 64 and 4096, on each bucket's n = 8192,
    12288 and 16384; and an all-0xff ciphertext of 4096 bytes."""
    names = list(S.ACC_TARGETS)
    lens = [n for _ in names for n in FORGE_NS] + [4096, 100]
    kidx = kidx_of(len(lens))
    in_off, out_off, pt_bytes, _ = slots(np.asarray(lens), 16)
    pt = bytearray(fp.sentinel(pt_bytes, 0x77).tobytes())
    for i, n in enumerate(lens):
        k = int(kidx[i])
        key, nonce = S.KEYS3[32 * k:32 * k + 32], S.tls_nonce(S.IVS3[12 * k:12 * k + 12], SEQ0 + i)
        ad = S.tls_ad(SEQ0 + i, n)
        if i < len(names) * len(FORGE_NS):
            name = names[i // len(FORGE_NS)]
            ct, tries = S.forge_ct(key, nonce, ad, n, S.ACC_TARGETS[name], f"mixed {name} {n}")
            assert tries <= 200 and S.accumulator(key, nonce, ad, ct) == S.ACC_TARGETS[name] % S.P
        elif n == 4096:
            ct = b"\xff" * n
        else:
            ct = S.rnd(n, "mixed forge filler")
        pt[int(in_off[i]):int(in_off[i]) + n] = R.xor_stream(key, nonce, ct)
    case = S.RfcCase(np.asarray(lens), bytes(pt), S.KEYS3, in_off=in_off, out_off=out_off, kidx=kidx, ivs_h=S.IVS3,
                     seq0=SEQ0)
    sealed = seal_open(case, ("forged",))
    lo, _ = case.out_range(len(lens) - 2)
    assert sealed[lo:lo + 4096] == b"\xff" * 4096
    r = last_routes()
    assert r["packed"] == 2 * len(names) + 1 and r["bucket"] == [len(names)] * 3 and r["classes"] == 1


# ---------------------------------------------------------------------------
# 6: neighbours on the library's workspace cache
# ---------------------------------------------------------------------------
def test_draft_calls_around_an_rfc_call(gpu, oracle, tamper_case):
    """draft, RFC, draft on the cached workspace: the oracle's bytes, the reference's,
    the oracle's again -- no n13 or IV stays behind in a slot, descriptor or table."""
    case = tamper_case
    draft = draft_twin(case)
    first = draft_seal_whole(draft, oracle, where=("before",))
    assert last_routes() == model_routes(draft, False)
    sealed = seal_open(case, ("between",))
    again = draft_seal_whole(draft, oracle, where=("after",))
    assert first == again and first != sealed
    assert S.seal_whole(case, where=("rfc again",)) == sealed
