"""TLS 1.3 record padding and per-record inner types on seal (sg_seal_batch_tls13_ex), and
the packed kernel in its TLS 1.3 form on seal and open, on the GPU.

The reference for every byte is tests/tls13_ref.py's seal(..., pad=); every buffer is
compared whole (tests/tls13_pad_support.py, tests/tls13_batch_support.py), so a record
must write exactly its inner + 16 bytes and read its input without changing it.  Every
switch a test sets is put back by gpu_support.kernel_forms."""
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
# content lengths: 62, 63 -> inner exactly 64 under pad_to 64 (63: no padding at all); 64: the type
# byte opens a block; 4094, 4095 -> inner 4096, the last packed size; 4096 -> 4160, the classes;
# 16384 -> the inner length is capped at 2^14 + 1
LENS = (0, 1, 15, 16, 17, 62, 63, 64, 126, 127, 128, 1000, 4094, 4095, 4096, 8191, 16383, 16384)
# ... and in an order whose records 0 and 16 -- the two that a layout skewed by odd bytes still
# leaves 16-byte aligned -- are too long for the packed kernel
SKEW_LENS = (4096,) + LENS[1:14] + (0,) + LENS[15:]
TYPES = (20, 21, 22, 23, 0xFF)
PADS = (64, 256, 100, 1)


def rnd(n, what):
    return S.rnd(n, what)


def ids(count, seq0=2**32 - 9):
    return np.arange(count, dtype=np.uint32) % 3, np.arange(count, dtype=np.uint64) + np.uint64(seq0)


@functools.lru_cache(maxsize=None)
def edge_records(lens=LENS):
    contents = [rnd(n, f"tls13 pad {i} {n}") for i, n in enumerate(lens)]
    kidx, seqs = ids(len(lens))
    types = [TYPES[i % len(TYPES)] for i in range(len(lens))]
    return contents, kidx, seqs, types


@functools.lru_cache(maxsize=None)
def edge_sealed(pad_to, lens=LENS):
    contents, kidx, seqs, types = edge_records(lens)
    return Q.expected_padded(contents, kidx, seqs, pad_to, types)


def packable(frags) -> int:
    """Fragments the packed kernel takes when every record is 16-byte aligned."""
    return sum(fp.pack_ok(len(f) - 16, 0, 0) for f in frags)


# ---------------------------------------------------------------------------
# 1. seal against the reference
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad_to", PADS)
def test_seal_against_the_reference(gpu, pad_to):
    contents, kidx, seqs, types = edge_records()
    want = edge_sealed(pad_to)
    images = []
    for pk in (1, 0):
        with kernel_forms(gpu, packed=pk):
            frags, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=pad_to, types=types, ctype=0, want=want,
                                                    where=("edges", pk))
            assert routes["known"] and routes["packed"] == (eligible if pk else 0), (pad_to, pk, routes)
        images.append(frags)
    assert images[0] == images[1] == want
    assert [len(f) for f in want] == [Q.inner_len(n, pad_to) + 16 for n in LENS]


@pytest.mark.parametrize("pad_to", [1, 0])
def test_no_padding_is_the_plain_seal(gpu, pad_to):
    """{NULL, 0 or 1, 0} is sg_seal_batch_tls13 byte for byte, routes included."""
    contents, kidx, seqs, _ = edge_records()
    want = X.expected_sealed(contents, kidx, seqs, 22)
    plain, r0, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=pad_to, ctype=22, plain=True, want=want, where=("plain",))
    ex, r1, _ = Q.seal_padded(contents, kidx, seqs, pad_to=pad_to, ctype=22, want=want, where=("ex",))
    assert plain == ex == want and r0 == r1
    # inner lengths 64 (63 content bytes), 128 (127) and 4096 (4095) are whole blocks without any padding
    assert eligible == 3
    expect_routes(r0, len(LENS), 3)


# ---------------------------------------------------------------------------
# 2. routes
# ---------------------------------------------------------------------------
def expect_routes(routes, count, packed):
    assert routes["known"] and routes["bucket"] == [0, 0, 0] and routes["skipped"] == 0, routes
    assert (routes["packed"], routes["classes"]) == (packed, count - packed), routes


def test_seal_routes(gpu):
    contents, kidx, seqs, _ = edge_records()
    _, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=64, want=None)
    assert eligible == sum(n <= 4095 for n in LENS) == 14
    expect_routes(routes, len(LENS), eligible)
    with kernel_forms(gpu, packed=0):
        _, routes, _ = Q.seal_padded(contents, kidx, seqs, pad_to=64)
        expect_routes(routes, len(LENS), 0)
    _, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=100)
    assert eligible == 0
    expect_routes(routes, len(LENS), 0)
    contents, kidx, seqs, _ = edge_records(SKEW_LENS)
    _, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=64, skew=(1, 3))
    assert eligible == 0
    expect_routes(routes, len(LENS), 0)


def test_open_routes(gpu):
    """Fragments as a peer that pads to 64 sends them, built by the reference."""
    contents, kidx, seqs, types = edge_records()
    want = [(T.OK, t, n) for t, n in zip(types, LENS)]
    frags = edge_sealed(64)
    got, routes = Q.open_routes(frags, kidx, seqs, where=("routes",))
    assert got == want and packable(frags) == 14
    expect_routes(routes, len(LENS), 14)
    with kernel_forms(gpu, packed=0):
        got, routes = Q.open_routes(frags, kidx, seqs, where=("routes", "packed off"))
        assert got == want
        expect_routes(routes, len(LENS), 0)
    frags = edge_sealed(100)
    assert packable(frags) == 0
    got, routes = Q.open_routes(frags, kidx, seqs, where=("routes", 100))
    assert got == want
    expect_routes(routes, len(LENS), 0)
    contents, kidx, seqs, types = edge_records(SKEW_LENS)
    got, routes = Q.open_routes(edge_sealed(64, SKEW_LENS), kidx, seqs, skew=(1, 3), where=("routes", "skewed"))
    assert got == [(T.OK, t, n) for t, n in zip(types, SKEW_LENS)]
    expect_routes(routes, len(LENS), 0)


# ---------------------------------------------------------------------------
# 3. run structure of the packed kernel
# ---------------------------------------------------------------------------
RUN_COUNT = 131                               # a run of 128 records and one of 3
RUN_INNER = (64, 128, 4096, 2112, 64, 1024)   # 117 blocks per six records: records straddle the 64-block chunks
RUN_ENDS = (0, 1, 15, 16, 17, 31, 32, 47, 48, 63)  # content bytes in the last block: bytes 0, 1 and 15 of every unit


def test_run_structure_padded_to_64(gpu):
    inners = [RUN_INNER[i % len(RUN_INNER)] for i in range(RUN_COUNT)]
    lens = [n - 64 + RUN_ENDS[i % len(RUN_ENDS)] for i, n in enumerate(inners)]
    assert [Q.inner_len(n, 64) for n in lens] == inners
    assert sum(inners[:128]) // 64 > 8 * 64  # the first run: more chunks than waves, so a second round
    contents = [rnd(n, f"tls13 run {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(RUN_COUNT, 2**32 - 70)
    types = [TYPES[i % len(TYPES)] for i in range(RUN_COUNT)]
    frags, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=64, types=types, where=("runs",))
    assert eligible == RUN_COUNT
    expect_routes(routes, RUN_COUNT, RUN_COUNT)
    got, routes = Q.open_routes(frags, kidx, seqs, where=("runs",))
    assert got == [(T.OK, t, n) for t, n in zip(types, lens)]
    expect_routes(routes, RUN_COUNT, RUN_COUNT)


def test_content_ends_in_every_part_of_the_record(gpu):
    """pad_to = 4096: every record is 64 blocks, and its content ends in the first, a middle
    or the last block, at byte 0, 1 and 15 of a 16-byte unit; lanes behind it load nothing."""
    lens = [b + e for b in (0, 64, 2048, 4032) for e in (0, 1, 15, 16, 17, 63) if b + e <= 4095] + [4095, 4079, 4080, 4081]
    contents = [rnd(n, f"tls13 ends {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(len(lens), 90)
    frags, routes, eligible = Q.seal_padded(contents, kidx, seqs, pad_to=4096, where=("ends",))
    assert eligible == len(lens) and all(len(f) == 4112 for f in frags)
    expect_routes(routes, len(lens), len(lens))
    got, routes = Q.open_routes(frags, kidx, seqs, where=("ends",))
    assert got == [(T.OK, 23, n) for n in lens]
    expect_routes(routes, len(lens), len(lens))


# ---------------------------------------------------------------------------
# 4. per-record types
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad_to", [64, 0])
def test_per_record_types(gpu, pad_to):
    lens = (0, 5, 63, 64, 100, 1000, 4095, 4096, 5000, 16384)
    contents = [rnd(n, f"tls13 types {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(len(lens), 2**40)
    types = [TYPES[i % len(TYPES)] for i in range(len(lens))]
    for pk in (1, 0):
        with kernel_forms(gpu, packed=pk):
            frags, _, _ = Q.seal_padded(contents, kidx, seqs, pad_to=pad_to, types=types, ctype=0, where=("types", pk))
            got = X.open_whole(frags, kidx, seqs, where=("types", pk))
            assert got == [(T.OK, t, n) for t, n in zip(types, lens)]


def test_per_record_types_of_uniform_full_records(gpu):
    """Full records in the wave-per-record kernel's shape: with inner_types the call stays
    off that route, whose pre-pass appends the call's one type."""
    from gpu_support import dev_u8
    from suruga_amd import batch as B

    count, M = 5, fp.MARGIN
    contents = [rnd(N, f"tls13 utypes {i}") for i in range(count)]
    kidx, seqs = ids(count, 77)
    types = list(TYPES)
    want = Q.expected_padded(contents, kidx, seqs, 64, types)
    case, in_size, out_size = X._case([N] * count, 17, kidx, seqs, (0, 0), (N, N + 32), X.IVS3, X.KEYS3, 19)
    in_img = np.concatenate([fp.sentinel(M, 0x31), fp.image(in_size, 0x77, zip(case.in_off, contents)), fp.sentinel(M, 0x32)])
    size = M + out_size + M
    rs = [(M + lo, M + hi) for lo, hi in map(case.out_range, range(count))]
    it = dev_u8(np.array(types, dtype=np.uint8))

    def call(d):
        batch = B.Batch(inp=d["inp"][M:], out=d["out"][M:], **case.seal_args())
        assert B.tls13_route(batch, False) == 1  # the plain seal of this batch takes the wave-per-record kernel
        B.seal_tls13(batch, pad_to=64, inner_types=it)

    o = fp.run_whole(call, in_img, fp.sentinel(size, 0x5A), fp.image(size, 0x5A, [(lo, w) for (lo, _), w in zip(rs, want)]), rs)
    o.check(where=("uniform types",))


# ---------------------------------------------------------------------------
# 5. open
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pad_to", [64, 256, 100])
def test_open_of_sealed_fragments(gpu, pad_to):
    contents, kidx, seqs, types = edge_records()
    want = [(T.OK, t, n) for t, n in zip(types, LENS)]
    for pk in (1, 0):
        with kernel_forms(gpu, packed=pk):
            assert X.open_whole(edge_sealed(pad_to), kidx, seqs, where=("open", pad_to, pk)) == want


def test_open_of_content_that_ends_in_zero_bytes(gpu):
    """Padded to 64 by the reference; the content's own trailing zeros stay content."""
    recs = [(rnd(40, "z0") + bytes(7), 23), (bytes(63), 22), (bytes(1), 21), (rnd(100, "z1") + bytes(27), 23),
            (rnd(4000, "z2") + bytes(95), 0xFF), (b"", 20), (rnd(64, "z3"), 23), (bytes(4095), 23)]
    kidx, seqs = ids(len(recs) + 1, 2**32 - 2)
    frags = [T.seal(*X.key_iv(int(kidx[i])), int(seqs[i]), c, t, Q.inner_len(len(c), 64) - len(c) - 1)
             for i, (c, t) in enumerate(recs)]
    frags.append(T.seal_inner(*X.key_iv(int(kidx[-1])), int(seqs[-1]), bytes(128)))  # a good tag over zeros alone
    want = [(T.OK, t, len(c)) for c, t in recs] + [(T.NO_TYPE, 0, 0)]
    assert packable(frags) == len(frags)
    for pk in (1, 0):
        with kernel_forms(gpu, packed=pk):
            got, routes = Q.open_routes(frags, kidx, seqs, where=("zeros", pk))
            assert got == want
            expect_routes(routes, len(frags), len(frags) if pk else 0)


# ---------------------------------------------------------------------------
# 6. tamper
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("pk", [1, 0], ids=["packed", "classes"])
@pytest.mark.parametrize("keep", [False, True], ids=["scrub", "keep"])
def test_tamper(gpu, keep, pk):
    count = 19
    inners = [(64, 192, 1024, 4096, 320)[i % 5] for i in range(count)]
    lens = [n - 64 + 30 for n in inners]  # 33 bytes of padding behind the type
    contents = [rnd(n, f"tls13 tamper {i}") for i, n in enumerate(lens)]
    kidx, seqs = ids(count, 2**32 - 10)
    sealed = Q.expected_padded(contents, kidx, seqs, 64, [23] * count)
    frags = [bytearray(f) for f in sealed]
    # the first ciphertext byte, a byte inside the padding, the last ciphertext byte, the tag's first and last byte
    flips = {1: (0, 0x01), 3: (lens[3] + 1 + 5, 0x40), 8: (inners[8] - 1, 0x80), 12: (inners[12], 0x01), 16: (inners[16] + 15, 0x80)}
    for i, (at, mask) in flips.items():
        frags[i][at] ^= mask
    with kernel_forms(gpu, packed=pk):
        got, routes = Q.open_routes([bytes(f) for f in frags], kidx, seqs, keep=keep, where=("tamper", pk, keep))
    assert got == [(T.BAD_MAC, 0, 0) if i in flips else (T.OK, 23, n) for i, n in enumerate(lens)]
    expect_routes(routes, count, count if pk else 0)


# ---------------------------------------------------------------------------
# 7. the MAC finish
# ---------------------------------------------------------------------------
def test_mac_finish(gpu):
    """Fragments whose ciphertext is all 0xff (one block and 64) under the reference's tag,
    and -- rfc_batch_support.forge_ct takes the 5-byte AD as it takes any -- fragments whose
    accumulator before the final reduction is == 0, p - 1, p, p + 4 and 2^130 - 1 (mod p),
    of one block, of 33 and of 64, through the packed TLS 1.3 form and through the classes."""
    shapes = [(64, None), (4096, None)] + [(n, k) for n in (64, 2112, 4096) for k in S.ACC_TARGETS]
    kidx, seqs = ids(len(shapes), 2**32 - 4)
    frags = []
    for i, (n, k) in enumerate(shapes):
        key, iv = X.key_iv(int(kidx[i]))
        nonce, ad = T.nonce(iv, int(seqs[i])), T.header(n + 16)
        ct = b"\xff" * n if k is None else S.forge_ct(key, nonce, ad, n, S.ACC_TARGETS[k], f"pad13 {n} {k}")[0]
        if k is not None:
            assert S.accumulator(key, nonce, ad, ct) == S.ACC_TARGETS[k] % S.P
        frags.append(ct + R.tag_of(key, nonce, ad, ct))
    for pk in (1, 0):
        with kernel_forms(gpu, packed=pk):
            got, routes = Q.open_routes(frags, kidx, seqs, where=("finish", pk))
            assert [g[0] for g in got] == [T.OK] * len(shapes)
            expect_routes(routes, len(shapes), len(shapes) if pk else 0)
    # a wrong tag over the same ciphertexts is still seen
    bad = [f[:-1] + bytes([f[-1] ^ 1]) for f in frags]
    got = X.open_whole(bad, kidx, seqs, where=("finish", "bad"))
    assert got == [(T.BAD_MAC, 0, 0)] * len(shapes)
