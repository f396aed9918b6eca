"""The 4-16 KiB wave-per-record buckets in TLS 1.3 form (sg_set_tls13_buckets), seal and
open, on the GPU.

The reference for every byte is tests/tls13_ref.py; every buffer is compared whole
(tests/tls13_pad_support.py, tests/tls13_batch_support.py), so a record writes exactly its
inner + 16 bytes and its input stays as it was.  The routes must be those of
tests/footprint.py's route model on the inner lengths (tls13_pad_support.routes_of).  The switch
is on unless a test says otherwise, and every switch a test sets is put back by
gpu_support.kernel_forms."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import footprint as fp
import rfc8439_ref as R
import rfc_batch_support as S
import tls13_batch_support as X
import tls13_pad_support as Q
import tls13_ref as T
from gpu_support import kernel_forms

pytestmark = pytest.mark.gpu

N = X.N
M = fp.MARGIN
TYPES = (20, 21, 22, 23, 0xFF)
NO_BUCKETS = [0, 0, 0]


def rnd(n, what):
    return S.rnd(n, what)


def ids(count, seq0=2**32 - 70):
    """Three keys in turn; sequence numbers that cross 2^32 within the batch."""
    return np.arange(count, dtype=np.uint32) % 3, np.arange(count, dtype=np.uint64) + np.uint64(seq0)


def types_of(count):
    return [TYPES[i % len(TYPES)] for i in range(count)]


# ---------------------------------------------------------------------------
# 1. edges against the reference, seal then open
# ---------------------------------------------------------------------------
# the bucket edges; then packed sizes (inner 64, 64, 1024, 4096), a bucket record with the most
# padding a pad_to of 64 gives (16320 -> 16384), a full record (inner 2^14 + 1: the classes) and 5000
EDGE_LENS = tuple(Q.bucket_edge_lens()) + (0, 63, 1000, 4095, 16320, 16384, 5000)


@functools.lru_cache(maxsize=None)
def edge_batch():
    contents = [rnd(n, f"tls13 bucket edge {i} {n}") for i, n in enumerate(EDGE_LENS)]
    kidx, seqs = ids(len(EDGE_LENS))
    types = types_of(len(EDGE_LENS))
    return contents, kidx, seqs, types, Q.expected_padded(contents, kidx, seqs, 64, types)


def test_edges_seal_then_open(gpu):
    contents, kidx, seqs, types, want = edge_batch()
    assert [len(w) - 16 for w in want[:len(Q.BUCKET_NS)]] == list(Q.BUCKET_NS)
    opened = [(T.OK, t, n) for t, n in zip(types, EDGE_LENS)]
    for on in (1, 0):
        with kernel_forms(gpu, tls13_buckets=on):
            frags, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=64, types=types, ctype=0, want=want,
                                                    where=("edges", on))
            model = Q.seal_routes(EDGE_LENS, 64, buckets=bool(on))
            assert frags == want and routes == model and eligible == model["packed"], (on, routes, model)
            got, routes = Q.open_routes(frags, kidx, seqs, where=("edges", on))
            assert got == opened and routes == Q.open_routes_of(frags, buckets=bool(on)), (on, routes)
            if on:
                assert model["bucket"] == [2 * 19 + 1, 2 * 19, 3 * 19 + 1] and routes["bucket"] == model["bucket"]
                assert model["packed"] == 4 and model["classes"] == 1
            else:
                assert routes["bucket"] == model["bucket"] == NO_BUCKETS and model["classes"] == len(EDGE_LENS) - 4


# ---------------------------------------------------------------------------
# 2. whole chunks of padding
# ---------------------------------------------------------------------------
# pad_to 8192: up to 8191 content bytes make 8192 inner bytes (J = 2), more make 2^14 (J = 4);
# pad_to 2^14: every record is 2^14 inner bytes.  The content ends in the first, a middle or the last
# chunk, at a chunk's first and last byte, or there is none; chunks behind it are padding alone.
PAD_LENS = {8192: (0, 1, 100, 4095, 4096, 4097, 5000, 8191, 8192, 8193, 9000, 12287, 12288, 12289, 16383, 16000),
            16384: (0, 1, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289, 16383, 17, 4111, 16368, 16369)}


@pytest.mark.parametrize("pad_to", sorted(PAD_LENS))
def test_whole_chunks_of_padding(gpu, pad_to):
    """The input slots lie back to back (tls13_pad_support.layout): the byte behind the aligned unit
    that holds a content's last byte is the next record's first, and the input image is compared
    whole; a record without content reads nothing."""
    lens = PAD_LENS[pad_to]
    contents = [rnd(n, f"tls13 chunks {pad_to} {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(len(lens), 2**32 - 5)
    types = types_of(len(lens))
    with kernel_forms(gpu, tls13_buckets=1):
        frags, routes, _ = Q.seal_padded(contents, kidx, seqs, pad_to=pad_to, types=types, ctype=0, where=("chunks",))
        model = Q.seal_routes(lens, pad_to, buckets=True)
        assert routes == model and model["classes"] == model["packed"] == 0, (routes, model)
        assert model["bucket"] == ([8, 0, 8] if pad_to == 8192 else [0, 0, 16])
        got, routes = Q.open_routes(frags, kidx, seqs, where=("chunks",))
        assert got == [(T.OK, t, n) for t, n in zip(types, lens)] and routes == model


# ---------------------------------------------------------------------------
# 3. eligibility
# ---------------------------------------------------------------------------
def test_eligibility_on_seal(gpu):
    # records 0 and 16, which a layout skewed by (1, 3) still leaves 16-byte aligned, are full records
    lens = [N if i in (0, 16) else n for i, n in enumerate(Q.bucket_edge_lens()[:21])]
    contents = [rnd(n, f"tls13 eligible {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(len(lens))
    with kernel_forms(gpu, tls13_buckets=1):
        _, routes, _ = Q.seal_padded(contents, kidx, seqs, pad_to=64, where=("aligned",))
        assert routes == Q.seal_routes(lens, 64, buckets=True) and sum(routes["bucket"]) == 19
        _, routes, _ = Q.seal_padded(contents, kidx, seqs, pad_to=64, skew=(1, 3), where=("skewed",))
        assert routes == Q.seal_routes(lens, 64, (1, 3), buckets=True) and routes["bucket"] == NO_BUCKETS, routes
        with kernel_forms(gpu, lockstep=0):
            _, routes, _ = Q.seal_padded(contents, kidx, seqs, pad_to=64, where=("lockstep off",))
            assert routes == Q.seal_routes(lens, 64, buckets=False) and routes["bucket"] == NO_BUCKETS, routes
        # multiples of 100 that are no multiples of 64
        assert all(Q.inner_len(n, 100) % 64 for n in lens)
        _, routes, _ = Q.seal_padded(contents, kidx, seqs, pad_to=100, where=("pad 100",))
        assert routes == Q.seal_routes(lens, 100, buckets=True) and routes["bucket"] == NO_BUCKETS, routes


def test_eligibility_on_open(gpu):
    """A full record's fragment (2^14 + 17 bytes) in a mixed batch stays on the size classes."""
    contents, kidx, seqs, types, want = edge_batch()
    pick = [0, 1, 2, 3, 4, 5, 6, len(EDGE_LENS) - 2, 7, 8]
    frags = [want[i] for i in pick]
    assert len(frags[7]) == N + 17
    opened = [(T.OK, types[i], EDGE_LENS[i]) for i in pick]
    with kernel_forms(gpu, tls13_buckets=1):
        got, routes = Q.open_routes(frags, kidx[pick], seqs[pick], where=("full",))
        assert got == opened and routes == Q.open_routes_of(frags, buckets=True)
        assert routes["classes"] == 1 and sum(routes["bucket"]) == 9, routes
        got, routes = Q.open_routes(frags, kidx[pick], seqs[pick], skew=(1, 3), where=("skewed",))
        assert got == opened and routes == Q.open_routes_of(frags, (1, 3), buckets=True)
        assert routes["bucket"] == [1, 0, 0], routes  # record 0 alone is still aligned
        with kernel_forms(gpu, lockstep=0):
            got, routes = Q.open_routes(frags, kidx[pick], seqs[pick], where=("lockstep off",))
            assert got == opened and routes["bucket"] == NO_BUCKETS, routes


# ---------------------------------------------------------------------------
# 4. a wave runs more than one record
# ---------------------------------------------------------------------------
def test_a_wave_runs_more_than_one_record(gpu):
    """One bucket (inner 4160), 8 (2 * 2 * CUs + 1) + 3 records: every workgroup of the persistent
    grid (two per CU) runs a second group, whose first chunk the first group's waves prefetch from
    the next record's content length, and the device counter hands out a third.  The whole images
    with the switch on are those with it off (the size classes), seal and open, and 16 sample
    records are the reference's."""
    import torch

    from suruga_amd import batch as B

    cus = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    count = 8 * (2 * 2 * cus + 1) + 3
    inner = 4160
    lens = [inner - 64 + Q.ENDS[i % len(Q.ENDS)] for i in range(count)]
    kidx, seqs = ids(count, 2**32 - 1000)
    types = types_of(count)
    in_off, out_off, in_size, out_size = Q.layout(lens, [inner] * count)
    rng = np.random.default_rng(4160)
    in_img = np.concatenate([fp.sentinel(M, 0x31), rng.integers(0, 256, in_size, dtype=np.uint8), fp.sentinel(M, 0x32)])
    case = X.Tls13Case(lens, None, X.KEYS3, in_off=in_off, out_off=out_off, kidx=kidx, seqs=seqs, ivs_h=X.IVS3,
                       content_type=0, version=(3, 3), tail=17)
    size = M + out_size + M
    rs = [(M + int(o), M + int(o) + inner + 16) for o in out_off]
    it = {}

    def seal(d):
        from gpu_support import dev_u8

        it["types"] = dev_u8(np.array(types, dtype=np.uint8))
        B.seal_tls13(B.Batch(inp=d["inp"][M:], out=d["out"][M:], **case.seal_args(max(lens))), pad_to=64, inner_types=it["types"])
        return B.last_routes()

    sealed = {}
    for on in (0, 1):
        with kernel_forms(gpu, tls13_buckets=on):
            o = fp.run_whole(seal, in_img, fp.sentinel(size, 0x5A), sealed.get(0), rs)
        assert o.ret["known"] and o.ret["bucket"] == ([count, 0, 0] if on else NO_BUCKETS), o.ret
        sealed[on] = o.out
        if on:
            o.check(where=("many", "seal"))  # the classes' image, and the input unchanged
        else:
            assert fp.first_diff(o.inp, in_img) is None
    rows = [int(i) for i in np.random.default_rng(16).choice(count, 16, replace=False)] + [0, count - 1]
    for i in rows:
        content = in_img[M + int(in_off[i]):M + int(in_off[i]) + lens[i]].tobytes()
        want = T.seal(*X.key_iv(int(kidx[i])), int(seqs[i]), content, types[i], inner - lens[i] - 1)
        assert sealed[1][rs[i][0]:rs[i][1]].tobytes() == want, ("many", "seal", i)

    # open: the sealed image is the input, fragment i at out_off[i]; the inner plaintext goes to a
    # slot of inner bytes rounded up to 16
    flens = np.full(count, inner + 16, dtype=np.uint32)
    pt_off = np.arange(count, dtype=np.uint64) * np.uint64(fp.round_up(inner, 16))
    ocase = X.Tls13Case([inner] * count, None, X.KEYS3, in_off=pt_off, out_off=out_off, kidx=kidx, seqs=seqs, ivs_h=X.IVS3,
                        content_type=23, version=(3, 3), tail=16)
    osize = M + count * fp.round_up(inner, 16) + M
    ors = [(M + int(o), M + int(o) + inner) for o in pt_off]

    def open_(d):
        B.open_tls13(B.Batch(inp=d["inp"][M:], out=d["out"][M:], status=d["status"], inner_type=d["inner_type"],
                             content_len=d["content_len"], **ocase.open_args(flens, inner + 16)))
        return B.last_routes()

    opened = {}
    for on in (0, 1):
        with kernel_forms(gpu, tls13_buckets=on):
            o = fp.run_whole(open_, sealed[1], fp.sentinel(osize, 0xA5), opened.get(0), ors,
                             arrays={"status": fp.array_start(count, 0x51), "inner_type": fp.array_start(count, 0x52),
                                     "content_len": fp.array_start(count, 0x53, np.uint32)})
        assert o.ret["known"] and o.ret["bucket"] == ([count, 0, 0] if on else NO_BUCKETS), o.ret
        opened[on] = o.out
        if on:
            o.check([T.OK] * count, types, lens, where=("many", "open"))
        else:
            assert fp.first_diff(o.inp, sealed[1]) is None
    for i in rows:
        content = in_img[M + int(in_off[i]):M + int(in_off[i]) + lens[i]].tobytes()
        want = content + bytes([types[i]]) + bytes(inner - lens[i] - 1)
        assert opened[1][ors[i][0]:ors[i][1]].tobytes() == want, ("many", "open", i)


# ---------------------------------------------------------------------------
# 5. tamper and scrub
# ---------------------------------------------------------------------------
TAMPER_INNER = (4160, 12288, 16384)  # J = 2, 3, 4


@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper(gpu, keep):
    """Every odd record is tampered with -- one of each bucket at the first ciphertext byte, inside
    the padding, at the last ciphertext byte, at the tag's first and at its last byte -- and every
    even one, its neighbours, opens intact."""
    count = 31
    inners = [TAMPER_INNER[(i // 2) % 3] for i in range(count)]
    lens = [n - 64 + 30 for n in inners]  # 33 bytes of padding behind the type
    contents = [rnd(n, f"tls13 bucket tamper {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(count, 2**32 - 10)
    frags = [bytearray(f) for f in Q.expected_padded(contents, kidx, seqs, 64, [23] * count)]
    flips = {}
    for i in range(1, count, 2):
        kind, n = (i // 2) // 3, inners[i]
        flips[i] = [(0, 0x01), (lens[i] + 1 + 5, 0x40), (n - 1, 0x80), (n, 0x01), (n + 15, 0x80)][kind]
        frags[i][flips[i][0]] ^= flips[i][1]
    assert len(flips) == 15
    with kernel_forms(gpu, tls13_buckets=1):
        got, routes = Q.open_routes([bytes(f) for f in frags], kidx, seqs, keep=keep, where=("tamper", keep))
    assert got == [(T.BAD_MAC, 0, 0) if i in flips else (T.OK, 23, n) for i, n in enumerate(lens)]
    assert routes == Q.open_routes_of(frags, buckets=True) and sum(routes["bucket"]) == count, routes


# ---------------------------------------------------------------------------
# 6. the MAC finish
# ---------------------------------------------------------------------------
def test_mac_finish(gpu):
    """Fragments whose ciphertext is all 0xff under the reference's tag, and fragments whose
    accumulator before the final reduction is == 0, p - 1, p, p + 4 and 2^130 - 1 (mod p)
    (rfc_batch_support.forge_ct with the 5-byte AD), of 2, 3 and 4 chunks, through the buckets and
    through the classes."""
    shapes = [(n, k) for n in (8192, 12288, 16384) for k in (None, *S.ACC_TARGETS)]
    kidx, seqs = ids(len(shapes), 2**32 - 4)
    frags = []
    for i, (n, k) in enumerate(shapes):
        key, iv = X.key_iv(int(kidx[i]))
        nonce, ad = T.nonce(iv, int(seqs[i])), T.header(n + 16)
        ct = b"\xff" * n if k is None else S.forge_ct(key, nonce, ad, n, S.ACC_TARGETS[k], f"bucket13 {n} {k}")[0]
        if k is not None:
            assert S.accumulator(key, nonce, ad, ct) == S.ACC_TARGETS[k] % S.P
        frags.append(ct + R.tag_of(key, nonce, ad, ct))
    bad = [f[:-1] + bytes([f[-1] ^ 1]) for f in frags]
    for on in (1, 0):
        with kernel_forms(gpu, tls13_buckets=on):
            got, routes = Q.open_routes(frags, kidx, seqs, where=("finish", on))
            assert [g[0] for g in got] == [T.OK] * len(shapes)
            assert routes["bucket"] == ([6, 6, 6] if on else NO_BUCKETS), routes
            # a wrong tag over the same ciphertexts is still seen
            got, routes = Q.open_routes(bad, kidx, seqs, where=("finish", "bad", on))
            assert got == [(T.BAD_MAC, 0, 0)] * len(shapes)
            assert routes["bucket"] == ([6, 6, 6] if on else NO_BUCKETS), routes


# ---------------------------------------------------------------------------
# 7. content that ends in zero bytes
# ---------------------------------------------------------------------------
def test_open_of_content_that_ends_in_zero_bytes(gpu):
    """Padded to 64 by the reference; the content's own trailing zeros stay content, and a good
    tag over 8192 zeros alone is SG_STATUS_NO_TYPE."""
    recs = [(rnd(8000, "bz0") + bytes(100), 23), (bytes(8191), 22), (rnd(5000, "bz1") + bytes(7), 0xFF),
            (bytes(4100), 21), (rnd(16300, "bz2") + bytes(83), 20)]
    kidx, seqs = ids(len(recs) + 1, 2**32 - 2)
    frags = [T.seal(*X.key_iv(int(kidx[i])), int(seqs[i]), c, t, Q.inner_len(len(c), 64) - len(c) - 1)
             for i, (c, t) in enumerate(recs)]
    frags.append(T.seal_inner(*X.key_iv(int(kidx[-1])), int(seqs[-1]), bytes(8192)))
    want = [(T.OK, t, len(c)) for c, t in recs] + [(T.NO_TYPE, 0, 0)]
    with kernel_forms(gpu, tls13_buckets=1):
        got, routes = Q.open_routes(frags, kidx, seqs, where=("zeros",))
    assert got == want
    assert routes == Q.open_routes_of(frags, buckets=True) and routes["bucket"] == [5, 0, 1], routes
