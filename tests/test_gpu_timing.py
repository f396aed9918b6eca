"""sg_set_timing / sg_timing_read on the GPU: one seal and one open of a batch on each
dispatch path give one seal window, one open window and two keying windows, all
longer than nothing; with timing off a read is empty; and switching timing on and off
many times with a batch in between changes neither the outputs nor the counts (the
library recycles its events through a pool: an event handed back twice would serve two
windows of a later batch at once).

The outputs are checked against the references once per case; the later runs are
compared with that first run."""
from __future__ import annotations

import functools

import numpy as np
import pytest

import footprint as fp
import gpu_support as G
import rfc_batch_support as S
import tls13_batch_support as X
import tls13_ref as T

pytestmark = pytest.mark.gpu

N = 1 << 14
COUNT = 9  # one full group of eight waves and one record more
LISTED_LENS = (0, 1, 64, 100, 4096, 4160, 16384)
TOGGLES = 50


@pytest.fixture
def timing(gpu):
    """set_timing(True) for the test; off again afterwards, whatever happened."""
    from suruga_amd import batch as B

    B.set_timing(True)
    try:
        yield B
    finally:
        B.set_timing(False)


def draft_uniform(oracle):
    """Nine full records, strides N and N + 16: the wave-per-record kernel."""
    from suruga_amd import batch as B

    keys = G.dev_bytes(G.KEY).view(1, 32)
    pt = G.uninit(COUNT * N)
    B.fill_records(pt, N, N, COUNT, G.SEED)
    ct, back, st = G.uninit(COUNT * (N + 16)), G.uninit(COUNT * N), G.filled(COUNT, 0xFF)
    assert all(t.data_ptr() % 16 == 0 for t in (pt, ct, back))
    pt_h = G.host_bytes(pt)
    want = oracle.seal_batch_tls(G.KEY, 5, pt_h, N, COUNT)

    def run():
        st.fill_(0xFF)
        B.seal(B.Batch(count=COUNT, keys=keys, inp=pt, out=ct, uniform_len=N, in_stride=N, out_stride=N + 16, seq0=5))
        B.open_(B.Batch(count=COUNT, keys=keys, inp=ct, out=back, uniform_len=N + 16, in_stride=N + 16, out_stride=N,
                        seq0=5, status=st))
        return G.host_bytes(ct), G.host_bytes(back), G.host_bytes(st)

    return run, (want, pt_h, bytes(COUNT))


@functools.lru_cache(maxsize=None)
def tls13_records():
    contents = [S.rnd(N, f"timing tls13 {i}") for i in range(COUNT)]
    kidx = np.arange(COUNT, dtype=np.uint32) % 3
    seqs = np.arange(COUNT, dtype=np.uint64) + np.uint64(2**32 - 4)
    return contents, kidx, seqs, X.expected_sealed(contents, kidx, seqs)


def tls13_uniform(oracle):
    """The same as TLS 1.3 records: 2^14 content bytes, fragments of 2^14 + 17."""
    from suruga_amd import batch as B

    contents, kidx, seqs, sealed = tls13_records()
    fs, bs = N + 32, N + 16  # fragment stride, inner-plaintext stride
    common = dict(count=COUNT, keys=G.dev_bytes(X.KEYS3).view(3, 32), ivs=G.dev_bytes(X.IVS3).view(3, 12),
                  key_index=G.dev_u32(kidx), seq=G.dev_u64(seqs))
    d_in, d_out, d_back = G.dev_bytes(b"".join(contents)), G.filled(COUNT * fs, 0), G.filled(COUNT * bs, 0)
    st, ty, cl = G.filled(COUNT, 0xFF), G.filled(COUNT, 0xFF), G.dev_u32([0xFFFFFFFF] * COUNT)
    seal = B.Batch(inp=d_in, out=d_out, uniform_len=N, in_stride=N, out_stride=fs, **common)
    open_ = B.Batch(inp=d_out, out=d_back, uniform_len=N + 17, in_stride=fs, out_stride=bs, status=st, inner_type=ty,
                    content_len=cl, **common)
    assert B.tls13_route(seal, False) == 1 and B.tls13_route(open_, True) == 1
    want_ct = b"".join(f.ljust(fs, b"\0") for f in sealed)
    want_back = b"".join((c + b"\x17").ljust(bs, b"\0") for c in contents)
    want_meta = bytes([T.OK] * COUNT) + bytes([23] * COUNT) + np.full(COUNT, N, dtype=np.uint32).tobytes()

    def run():
        st.fill_(0xFF)
        B.seal_tls13(seal)
        B.open_tls13(open_)
        return G.host_bytes(d_out), G.host_bytes(d_back), G.host_bytes(st) + G.host_bytes(ty) + G.host_bytes(cl)

    return run, (want_ct, want_back, want_meta)


def draft_listed(oracle):
    """A listed TLS batch whose records take the size classes, the packed kernel and
    two buckets."""
    from suruga_amd import batch as B

    lens = np.array(LISTED_LENS)
    in_off, out_off, pt_bytes, ct_bytes = G.slots(lens, 16)
    pt_h = S.rnd(pt_bytes, "timing listed")
    case = G.BatchCase(lens, pt_h, in_off=in_off, out_off=out_off, seq0=11)
    want_routes = fp.route_counts(lens, in_off, out_off, *fp.mixed_routes(int(lens.max()), True, True))
    assert {k[0] for k in want_routes} == {"class", "packed", "bucket"}
    d_in, d_out, d_back = G.dev_u8(np.frombuffer(pt_h, dtype=np.uint8)), G.filled(ct_bytes, 0), G.filled(pt_bytes, 0)
    want_ct = bytes(case.sealed_image(oracle, ct_bytes))
    want_back = bytearray(pt_bytes)
    for i in range(case.count):
        want_back[int(in_off[i]):int(in_off[i]) + case.n(i)] = case.pt(i)

    def run():
        ct = G.seal(case, d_out, inp=d_in)
        r = B.last_routes()
        assert r["known"] and r["skipped"] == 0, r
        got = {("class",): r["classes"], ("packed",): r["packed"], ("bucket",): sum(r["bucket"])}
        assert got == {k: sum(v for q, v in want_routes.items() if q[0] == k[0]) for k in got}, (r, want_routes)
        back, st = G.open_(case, d_out, d_back)
        return bytes(ct), back, st

    return run, (want_ct, bytes(want_back), bytes(case.count))


CASES = {"draft-wpr": draft_uniform, "tls13-wpr": tls13_uniform, "draft-listed": draft_listed}


def read_one_pair(B, where):
    """The windows of one seal and one open."""
    t = B.timing_read()
    assert (t["n_seal"], t["n_open"], t["n_keying"]) == (1, 1, 2), (*where, t)
    assert t["seal_ms"] > 0 and t["open_ms"] > 0 and t["keying_ms"] > 0, (*where, t)


@pytest.mark.parametrize("name", list(CASES))
def test_one_seal_and_one_open_are_three_windows(timing, oracle, name):
    B = timing
    run, want = CASES[name](oracle)
    got = run()
    for what, g, w in zip(("sealed", "opened", "status"), got, want):
        assert g == w, (name, what)
    read_one_pair(B, (name,))
    B.set_timing(False)
    assert B.timing_read() == {"seal_ms": 0.0, "open_ms": 0.0, "keying_ms": 0.0, "n_seal": 0, "n_open": 0, "n_keying": 0}


@pytest.mark.parametrize("name", list(CASES))
def test_toggling_timing_leaves_results_and_counts_alone(timing, oracle, name):
    B = timing
    run, want = CASES[name](oracle)
    first = run()
    assert first == want, name
    read_one_pair(B, (name, "first"))
    for k in range(TOGGLES):
        B.set_timing(False)  # hands the events of the last pair back
        B.set_timing(True)
        assert run() == first, (name, k)
        read_one_pair(B, (name, k))
