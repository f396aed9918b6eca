"""The record layer over host memory in TLS 1.3 and RFC 7905 on the GPU:
sg_write_records_tls13 / _rfc7905 against the batch calls and record13_ref,
sg_read_records_tls13 / _rfc7905 against record13_ref's expected read, on pageable
and on registered buffers, in both kernel forms where full records occur and with
SG_RECORD13_GATHER at both values; every buffer inside sentinel margins."""
from __future__ import annotations

import ctypes as C
import functools
import random
import socket
import threading

import numpy as np
import pytest

import record13_ref as RR
import record13_support as S
from gpu_support import kernel_forms

pytestmark = pytest.mark.gpu
FULL = RR.FULL


def _nrec(n):
    return (n + FULL - 1) // FULL


def _bound(form, n):
    return n + (22 if form == "tls13" else 21) * _nrec(n)


def _fragments(data: bytes):
    return [data[o:o + FULL] for o in range(0, len(data), FULL)]


# ---------------------------------------------------------------------------
# write
# ---------------------------------------------------------------------------
def _write_case(gpu, form, n, reg, woff=0, seq0=7, ctype=23):
    data = RR.content(n, f"w{form}")
    frs = _fragments(data)
    want = S.framed(form, ctype, S.batch_fragments(gpu, form, seq0, ctype, frs))
    assert len(want) == _bound(form, n)
    # a seeded sample against the reference: the first and last record and both sides of the chunk seam
    idx = {0, len(frs) - 1} | ({255, 256} & set(range(len(frs))))
    rnd = random.Random(n)
    while len(idx) < min(8, len(frs)):
        idx.add(rnd.randrange(len(frs)))
    pitch = 5 + FULL + (17 if form == "tls13" else 16)
    for i in sorted(idx):
        rec = S.ref_record(form, seq0 + i, ctype, frs[i])
        assert want[i * pitch:i * pitch + len(rec)] == rec, (form, n, i)
    d, w = S.Buf(n, 0, 0x21, fill=data), S.Buf(len(want), woff, 0x43)
    with S.context(gpu) as ctx, S.registered(gpu, (d, w), reg):
        images = []
        for ls in ((0, 1) if n >= FULL else (1,)):
            w.reset()
            with kernel_forms(gpu, lockstep=ls):
                rc, wl = S.write(gpu, form, ctx, seq0, ctype, d, w)
            assert (rc, wl) == (len(frs), len(want)), (form, n, reg, ls)
            w.check(want, f"{form} write n={n} registered={reg} lockstep={ls} offset={woff}")
            d.check(data, "the data buffer")
            images.append(w.arr.copy())
        assert all(np.array_equal(images[0], im) for im in images)


@pytest.mark.parametrize("reg", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("n", [1, FULL - 1, FULL, FULL + 1, 2 * FULL + 5])
def test_write_lengths(gpu, form, n, reg):
    _write_case(gpu, form, n, reg)


@pytest.mark.parametrize("reg", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("form", S.FORMS)
def test_write_across_the_chunk_seam(gpu, form, reg):
    _write_case(gpu, form, 257 * FULL + 3, reg)


@pytest.mark.parametrize("form", S.FORMS)
@pytest.mark.parametrize("woff", [1, 2, 3])
def test_write_into_a_misaligned_wire(gpu, form, woff):
    _write_case(gpu, form, FULL + 5, True, woff=woff)
    _write_case(gpu, form, 37, False, woff=woff)


@pytest.mark.parametrize("form", S.FORMS)
def test_write_nothing(gpu, form):
    d, w = S.Buf(16), S.Buf(64)
    d.hi = d.lo  # len == 0
    with S.context(gpu) as ctx:
        assert S.write(gpu, form, ctx, 0, 23, d, w) == (0, 0)
        w.check(b"", "len == 0 leaves the wire untouched")
        if form == "tls13":
            from suruga_amd import _native as N

            d.hi = d.lo + 16
            assert S.write(gpu, form, ctx, 0, 0, d, w)[0] == N.SG_E_ARG  # a zero inner type
            w.check(b"", "a refused call leaves the wire untouched")


# ---------------------------------------------------------------------------
# read, TLS 1.3
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream(name: str) -> RR.Stream:
    if name in ("mixed", "mixed-cut"):
        pads = (0, 1, 15, 16, 255)
        items = [RR.Item(RR.content(n, f"m{i}"), (21, 22, 23)[i % 3], pads[i % 5])
                 for i, n in enumerate((1, 2, 3, 4, 5, 0, 17, 100, 333, 4096, 0, 63, 64, FULL, 65, 5000, 1, 0, 7))]
        # (the full record carries 16 bytes of padding: 2^14 + 1 + 16 + 16 <= 2^14 + 256)
        return RR.stream13(items, seq0=3, cut=9 if name == "mixed-cut" else 0)
    if name == "full257":
        return RR.stream13([RR.Item(RR.content(FULL, f"f{i}")) for i in range(257)], seq0=1 << 40)
    if name == "small1025":
        return RR.stream13([RR.Item(RR.content(64, f"s{i}"), (21, 22, 23)[i % 3]) for i in range(1025)])
    raise KeyError(name)


def _read_case(gpu, form, st, reg, ooff, what, lockstep=(1,), gathers=(0, 1), seq0=0, slack=0):
    want = RR.expected_read(st)
    cap = (RR.out_capacity13(st) if form == "tls13" else sum(len(it.content) for it in st.items)) + slack
    w, o = S.Buf(len(st.wire), 0, 0x11, fill=st.wire), S.Buf(cap, ooff, 0x6C)
    with S.context(gpu) as ctx, S.registered(gpu, (w, o), reg):
        for ls in lockstep:
            for g in gathers:
                o.reset()
                prev = gpu.sg_set_record13_gather(g)
                try:
                    with kernel_forms(gpu, lockstep=ls):
                        got = S.read(gpu, form, ctx, seq0, w, o, max_records=len(st.items) + 3)
                finally:
                    gpu.sg_set_record13_gather(prev)
                tag = f"{what} registered={reg} lockstep={ls} gather={g} offset={ooff}"
                S.check_read(got, want, tag)
                # beyond out_len: the sentinel or zero, never plaintext; outside the window: untouched
                o.check(want.out, tag, zero_ok_from=want.out_len)
                w.check(st.wire, "the wire buffer")
    return want


@pytest.mark.parametrize("reg", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("ooff", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["mixed", "mixed-cut"])
def test_read_tls13_mixed_records(gpu, name, ooff, reg):
    st = _stream(name)
    want = _read_case(gpu, "tls13", st, reg, ooff, name, seq0=3)
    assert want.records == (19 if name == "mixed" else 18) and want.error == RR.OK
    assert set(want.types) == {21, 22, 23} and 0 in want.lens


@pytest.mark.parametrize("reg", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("ooff", [0, 3])
def test_read_tls13_full_records_across_the_seam(gpu, ooff, reg):
    want = _read_case(gpu, "tls13", _stream("full257"), reg, ooff, "257 full records", lockstep=(0, 1), seq0=1 << 40)
    assert want.records == 257 and want.out_len == 257 * FULL


@pytest.mark.parametrize("reg", [False, True], ids=["pageable", "registered"])
def test_read_tls13_five_chunks_reuse_the_slots(gpu, reg):
    want = _read_case(gpu, "tls13", _stream("small1025"), reg, 1, "1025 records of 64 bytes")
    assert want.records == 1025 and want.out_len == 1025 * 64


# ---------------------------------------------------------------------------
# read failures: each composed as data
# ---------------------------------------------------------------------------
FAIL_N = 300


@functools.lru_cache(maxsize=None)
def _good(i: int) -> bytes:
    return RR.content(48, f"g{i}")


@functools.lru_cache(maxsize=None)
def _fail_stream(pos: int, kind: str) -> RR.Stream:
    items = [RR.Item(_good(i)) for i in range(FAIL_N)]
    if kind == "long":
        items[pos] = RR.failing("long", f"L{pos}")
    else:  # the same length as its neighbours: the chunk stays equal and dense (zero-copy when registered)
        items[pos] = RR.Item(_good(pos), fail=kind)
    return RR.stream13(items, seq0=11)


@pytest.mark.parametrize("kind,err", [("tag", RR.E_BAD_MAC), ("zeros", RR.E_UNEXPECTED_MESSAGE),
                                      ("long", RR.E_RECORD_OVERFLOW)])
@pytest.mark.parametrize("pos", [0, 100, 255, 256])
def test_read_tls13_stops_at_the_failing_record(gpu, pos, kind, err):
    st = _fail_stream(pos, kind)
    for reg in (False, True):
        want = _read_case(gpu, "tls13", st, reg, 1, f"{kind} at record {pos}", seq0=11)
        assert (want.records, want.error, want.out_len) == (pos, err, 48 * pos)


def test_read_tls13_failure_leaves_no_later_plaintext(gpu):
    """The plaintext of the failing record and of the records behind it appears
    nowhere in `out`, window and margins alike."""
    for kind in ("tag", "long"):
        st = _fail_stream(100, kind)
        w = S.Buf(len(st.wire), 0, 0x11, fill=st.wire)
        for reg in (False, True):
            for g in (0, 1):
                o = S.Buf(RR.out_capacity13(st), 2, 0x6C)
                prev = gpu.sg_set_record13_gather(g)
                try:
                    with S.context(gpu) as ctx, S.registered(gpu, (w, o), reg):
                        got = S.read(gpu, "tls13", ctx, 11, w, o, max_records=FAIL_N)
                finally:
                    gpu.sg_set_record13_gather(prev)
                assert got.records == 100
                image = o.arr.tobytes()
                for j in (100, 101, 255, 256, FAIL_N - 1):
                    c = st.items[j].content
                    assert c[:16] not in image and c[-16:] not in image, (kind, reg, g, j)


# ---------------------------------------------------------------------------
# read, RFC 7905
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stream7905(name: str) -> RR.Stream:
    if name == "seam":
        return RR.stream7905([RR.Item(RR.content(48, f"r{i}")) for i in range(FAIL_N)], seq0=5)
    if name == "mixed":  # types and versions differ inside the chunk: explicit mode, nonces built on the host
        return RR.stream7905([RR.Item(RR.content(10 + 7 * i, f"x{i}"), (20, 21, 22, 23)[i % 4], version=(3, 1 + i % 3))
                              for i in range(40)], seq0=(1 << 32) - 20)
    if name == "tampered":
        items = [RR.Item(RR.content(48, f"r{i}")) for i in range(FAIL_N)]
        items[256] = RR.Item(items[256].content, fail="tag")
        return RR.stream7905(items, seq0=5)
    if name == "full":
        return RR.stream7905([RR.Item(RR.content(FULL, f"f{i}")) for i in range(6)], seq0=9, cut=100)
    raise KeyError(name)


@pytest.mark.parametrize("reg", [False, True], ids=["pageable", "registered"])
@pytest.mark.parametrize("name,seq0,records,err", [("seam", 5, FAIL_N, RR.OK), ("mixed", (1 << 32) - 20, 40, RR.OK),
                                                   ("tampered", 5, 256, RR.E_BAD_MAC), ("full", 9, 5, RR.OK)])
def test_read_rfc7905(gpu, name, seq0, records, err, reg):
    st = _stream7905(name)
    want = _read_case(gpu, "rfc7905", st, reg, 1, name, lockstep=(0, 1) if name == "full" else (1,), gathers=(0,),
                      seq0=seq0)
    assert (want.records, want.error) == (records, err)


# ---------------------------------------------------------------------------
# no IV, round trip, concurrency
# ---------------------------------------------------------------------------
def test_calls_without_an_iv_are_refused_and_touch_nothing(gpu):
    from suruga_amd import _native as N

    st = _stream("mixed")
    d, w, o = S.Buf(100, 0, 1, fill=RR.content(100)), S.Buf(len(st.wire), 0, 2, fill=st.wire), S.Buf(70000, 0, 3)
    res = N.SgReadResult()
    res.records, res.error = 77, 9
    with S.context(gpu, iv=None) as ctx:
        for form in S.FORMS:
            wl = C.c_size_t(5)
            args = (ctx, 0, 23) + ((3, 3) if form == "rfc7905" else ()) + (d.ptr, d.n, o.ptr, o.n, C.byref(wl))
            fn = gpu.sg_write_records_tls13 if form == "tls13" else gpu.sg_write_records_rfc7905
            assert fn(*args) == N.SG_E_ARG and wl.value == 5
            assert b"sg_ctx_set_iv" in gpu.sg_last_error()
            fn = gpu.sg_read_records_tls13 if form == "tls13" else gpu.sg_read_records_rfc7905
            assert fn(ctx, 0, w.ptr, w.n, o.ptr, o.n, None, None, 64, C.byref(res)) == N.SG_E_ARG
            assert (res.records, res.error) == (77, 9)
            o.check(b"", "a refused call leaves out untouched")
        # the draft calls on the same context are as before
        wl = C.c_size_t(0)
        assert gpu.sg_write_records(ctx, 0, 23, 3, 3, d.ptr, d.n, o.ptr, o.n, C.byref(wl)) == 1 and wl.value == 121


def test_writer_to_reader_over_a_socketpair(gpu):
    from suruga_amd.tls13 import Tls13StreamReader, Tls13Writer

    a, b = socket.socketpair()
    data = RR.content(3 * FULL + 7, "rt")
    wr, rd = Tls13Writer(a, RR.KEY, RR.IV), Tls13StreamReader(RR.KEY, RR.IV)
    try:
        t = threading.Thread(target=lambda: (wr.write_application_data(data), wr.write_alert(1, 0), a.close()))
        t.start()
        msgs = []
        while True:
            chunk = b.recv(1 << 16)
            if not chunk:
                break
            rd.feed(chunk)
            msgs += rd.drain()
        t.join()
        assert wr.write_count == 5 and rd.read_count == 5 and not rd.buf
        assert [ty for ty, _ in msgs] == [23, 23, 23, 23, 21]
        assert b"".join(m for ty, m in msgs if ty == 23) == data and msgs[-1][1] == b"\x01\x00"
    finally:
        b.close()
        wr.close()
        rd.close()


def test_rfc7905_encryptor_routes_through_tls_py(gpu):
    import io

    from suruga_amd.cipher import ChaCha20Poly1305Rfc7905Decryptor, ChaCha20Poly1305Rfc7905Encryptor
    from suruga_amd.tls import ContentType, RecordStreamReader, TlsWriter

    sink = io.BytesIO()
    wr = TlsWriter(sink)
    wr.set_encryptor(ChaCha20Poly1305Rfc7905Encryptor(RR.KEY, RR.IV))
    data = RR.content(FULL + 9, "tlspy")
    wr.write_application_data(data)
    wire = sink.getvalue()
    want = b"".join(S.ref_record("rfc7905", i, 23, f) for i, f in enumerate(_fragments(data)))
    assert wire == want and wr.write_count == 2
    rd = RecordStreamReader(None, ChaCha20Poly1305Rfc7905Decryptor(RR.KEY, RR.IV), max_records=16)
    rd.feed(wire)
    assert rd.drain() == [(ContentType.ApplicationDataTy, data[:FULL]), (ContentType.ApplicationDataTy, data[FULL:])]


def test_writer_and_reader_on_two_contexts_in_two_threads(gpu):
    n = 64 * FULL
    data = RR.content(n, "conc")
    other = RR.content(n, "conc2")
    with S.context(gpu) as wctx, S.context(gpu) as rctx:
        d, w = S.Buf(n, 0, 1, fill=data), S.Buf(_bound("tls13", n), 0, 2)
        assert S.write(gpu, "tls13", wctx, 0, 23, d, w) == (64, w.n)
        serial_wire = w.window().tobytes()
        o = S.Buf(n, 0, 3)
        serial = S.read(gpu, "tls13", rctx, 0, w, o, max_records=64)
        assert serial.out == data and serial.records == 64
        # now both at once: the writer seals other data while the reader opens the first wire
        d2, w2, o2 = S.Buf(n, 0, 4, fill=other), S.Buf(w.n, 0, 5), S.Buf(n, 0, 6)
        results = {}
        ts = [threading.Thread(target=lambda: results.__setitem__("w", S.write(gpu, "tls13", wctx, 0, 23, d2, w2))),
              threading.Thread(target=lambda: results.__setitem__("r", S.read(gpu, "tls13", rctx, 0, w, o2, 64)))]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert results["w"] == (64, w.n)
        S.check_read(results["r"], serial, "concurrent read")
        w.reset()
        assert S.write(gpu, "tls13", wctx, 0, 23, d2, w) == (64, w.n)  # the serial run of the second write
        assert w2.window().tobytes() == w.window().tobytes() != serial_wire
