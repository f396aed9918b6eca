"""The host-only part of the TLS 1.3 record layer: sg_wire_bound_tls13 and
sg_parse_records_tls13 (every check, in order), and the calls that need the
context's write IV refusing a NULL context before any GPU work.  CPU only."""
from __future__ import annotations

import ctypes as C
import struct

import pytest

import record13_ref as RR

FULL = 1 << 14


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


@pytest.mark.parametrize("n", [0, 1, FULL - 1, FULL, FULL + 1, 3 * FULL])
def test_wire_bound_tls13(lib, n):
    assert lib.sg_wire_bound_tls13(n) == n + 22 * ((n + FULL - 1) // FULL) == RR.wire_bound13(n)


def parse(lib, wire: bytes, max_records: int = 64):
    from suruga_amd import _native as N

    recs = (N.SgWireRecord * max_records)()
    count, err = C.c_size_t(0), C.c_int32(0)
    buf = (C.c_uint8 * max(len(wire), 1)).from_buffer_copy(wire or b"\0")
    assert lib.sg_parse_records_tls13(buf, len(wire), max_records, recs, C.byref(count), C.byref(err)) == N.SG_OK
    return [(r.offset, r.frag_len, r.type, r.ver_major, r.ver_minor) for r in recs[:count.value]], err.value


def rec(ty: int, flen: int, version=(3, 3)) -> bytes:
    return struct.pack(">BBBH", ty, version[0], version[1], flen) + bytes(flen)


@pytest.mark.parametrize("ty", [20, 21, 22, 24])
def test_outer_type_other_than_23_is_unexpected_message(lib, ty):
    good = rec(23, 40)
    assert parse(lib, good + rec(ty, 40)) == ([(5, 40, 23, 3, 3)], RR.E_UNEXPECTED_MESSAGE)
    # the type is checked first: with an oversize or a short length too
    assert parse(lib, struct.pack(">BBBH", ty, 3, 3, 0xFFFF)) == ([], RR.E_UNEXPECTED_MESSAGE)
    assert parse(lib, struct.pack(">BBBH", ty, 3, 3, 3) + bytes(3)) == ([], RR.E_UNEXPECTED_MESSAGE)


@pytest.mark.parametrize("flen,err", [(15, RR.E_SHORT), (16, RR.OK), (17, RR.OK), (FULL + 256, RR.OK),
                                      (FULL + 257, RR.E_RECORD_OVERFLOW)])
def test_length_limits(lib, flen, err):
    recs, e = parse(lib, rec(23, 100) + rec(23, flen))
    assert e == err
    assert recs == [(5, 100, 23, 3, 3)] + ([(110, flen, 23, 3, 3)] if err == RR.OK else [])


def test_overflow_is_checked_before_completeness_and_short_after(lib):
    # an oversize length is an error even when the record's bytes have not arrived
    assert parse(lib, struct.pack(">BBBH", 23, 3, 3, FULL + 257)) == ([], RR.E_RECORD_OVERFLOW)
    # a short length whose bytes have not arrived is an incomplete record, no error yet
    assert parse(lib, struct.pack(">BBBH", 23, 3, 3, 15) + bytes(14)) == ([], RR.OK)
    assert parse(lib, struct.pack(">BBBH", 23, 3, 3, 15) + bytes(15)) == ([], RR.E_SHORT)


def test_truncated_last_record_and_headers(lib):
    whole = rec(23, 50) + rec(23, 60)
    for cut in (1, 59, 60, 61, 64):  # inside the fragment, at its start, inside the header
        recs, e = parse(lib, whole[:len(whole) - cut])
        assert (recs, e) == ([(5, 50, 23, 3, 3)], RR.OK), cut
    assert parse(lib, whole) == ([(5, 50, 23, 3, 3), (60, 60, 23, 3, 3)], RR.OK)
    assert parse(lib, b"") == ([], RR.OK)
    assert parse(lib, whole, max_records=1) == ([(5, 50, 23, 3, 3)], RR.OK)


def test_version_bytes_are_reported_not_checked(lib):
    assert parse(lib, rec(23, 30, (3, 1)) + rec(23, 30, (9, 9))) == ([(5, 30, 23, 3, 1), (40, 30, 23, 9, 9)], RR.OK)


def test_parse_matches_reference_stream(lib):
    st = RR.stream13([RR.Item(RR.content(10), 23), RR.Item(b"", 21, pad=16), RR.Item(RR.content(300), 22, pad=255)])
    recs, e = parse(lib, st.wire)
    assert e == RR.OK and [r[0] - 5 for r in recs] == st.offsets[:-1]
    assert [r[1] for r in recs] == [27, 33, 300 + 1 + 255 + 16]


def test_argument_errors_without_gpu(lib):
    from suruga_amd import _native as N

    wl = C.c_size_t(7)
    buf = (C.c_uint8 * 64)()
    res = N.SgReadResult()
    assert lib.sg_ctx_set_iv(None, bytes(12)) == N.SG_E_ARG
    assert lib.sg_write_records_tls13(None, 0, 23, buf, 1, buf, 64, C.byref(wl)) == N.SG_E_ARG
    assert lib.sg_write_records_rfc7905(None, 0, 23, 3, 3, buf, 1, buf, 64, C.byref(wl)) == N.SG_E_ARG
    assert lib.sg_read_records_tls13(None, 0, buf, 10, buf, 64, None, None, 4, C.byref(res)) == N.SG_E_ARG
    assert lib.sg_read_records_rfc7905(None, 0, buf, 10, buf, 64, None, None, 4, C.byref(res)) == N.SG_E_ARG
    assert wl.value == 7
    cur = (N.SgGatherCursor * 2)()
    r2 = (C.c_uint32 * 2)()
    assert lib.sg_gather_records(None, 18432, None, None, 257, None, 0, cur, C.byref(cur[1]), r2, None) == N.SG_E_ARG
    assert lib.sg_gather_records(None, 18432, None, None, 4, None, 0, cur, C.byref(cur[1]), r2, None) == N.SG_E_ARG
    assert lib.sg_set_record13_gather(-1) in (0, 1)
