"""tests/record13_ref.py pinned against OpenSSL's stored records
(tests/golden/tls13_records.json, tests/golden/rfc7905_records.json), and its
expected read result checked on streams small enough to read by eye.  CPU only."""
from __future__ import annotations

import hashlib
import json

import pytest

import record13_ref as RR
import rfc8439_ref as R
from conftest import GOLDEN


def _golden(name):
    return json.loads((GOLDEN / name).read_text())


def test_tls13_records_equal_openssl():
    g = _golden("tls13_records.json")
    key, ivs = bytes.fromhex(g["key"]), [bytes.fromhex(x) for x in g["ivs"]]
    for c in g["cases"]:
        it = RR.Item(R.data(c["n"], b"tls13 content %d" % c["n"]), g["type"], c["pad"])
        rec = RR.record13(key, ivs[c["iv"]], c["seq"], it)
        assert rec[:5].hex() == c["ad"], c
        assert rec[-16:].hex() == c["tag"], c
        assert hashlib.sha256(rec[5:-16]).hexdigest() == c["ct_sha256"], c
        assert len(rec) == 5 + c["n"] + 1 + c["pad"] + 16


def test_rfc7905_records_equal_openssl():
    g = _golden("rfc7905_records.json")
    key, ivs = bytes.fromhex(g["key"]), [bytes.fromhex(x) for x in g["ivs"]]
    major, minor, ctype = 3, 3, 23
    # (the fixture's header is type 23, version 3.3: every case's ad field pins it below)
    for c in g["cases"]:
        it = RR.Item(R.data(c["n"], b"rfc7905 pt %d" % c["n"]), ctype, version=(major, minor))
        rec = RR.record7905(key, ivs[c["iv"]], c["seq"], it)
        assert bytes.fromhex(c["ad"])[8:11] == rec[:3], c
        assert rec[-16:].hex() == c["tag"], c
        assert hashlib.sha256(rec[5:-16]).hexdigest() == c["ct_sha256"], c
        assert int.from_bytes(rec[3:5], "big") == c["n"] + 16


def test_wire_bound():
    for n, want in ((0, 0), (1, 23), (RR.FULL, RR.PITCH13), (RR.FULL + 1, RR.PITCH13 + 23)):
        assert RR.wire_bound13(n) == want


def _items():
    return [RR.Item(RR.content(10, "a"), 23), RR.Item(b"", 21, pad=3), RR.Item(RR.content(7, "b"), 22, pad=1)]


def test_expected_read_delivers_everything():
    st = RR.stream13(_items())
    r = RR.expected_read(st)
    assert (r.records, r.error, r.types, r.lens) == (3, RR.OK, [23, 21, 22], [10, 0, 7])
    assert r.consumed == len(st.wire) == (5 + 27) + (5 + 20) + (5 + 25)
    assert r.out == RR.content(10, "a") + RR.content(7, "b") and r.out_len == 17
    assert RR.out_capacity13(st) == 10 + 3 + 8


@pytest.mark.parametrize("kind,err", [("tag", RR.E_BAD_MAC), ("zeros", RR.E_UNEXPECTED_MESSAGE),
                                      ("long", RR.E_RECORD_OVERFLOW)])
def test_expected_read_stops_at_the_failing_record(kind, err):
    items = _items()
    items.insert(1, RR.failing(kind))
    st = RR.stream13(items)
    r = RR.expected_read(st)
    assert (r.records, r.error, r.types, r.lens, r.out) == (1, err, [23], [10], RR.content(10, "a"))
    assert r.consumed == st.offsets[1]


def test_failing_records_are_what_they_claim():
    """Each failing kind against tls13_ref.open: the tag fails, the all-zero inner is
    authentic and has no type, the long content is authentic."""
    import tls13_ref as T

    for seq, kind in enumerate(("tag", "zeros", "long")):
        rec = RR.record13(RR.KEY, RR.IV, seq, RR.failing(kind))
        st, _, ty, n = T.open(RR.KEY, RR.IV, seq, rec[5:])
        assert (st, ty, n) == {"tag": (T.BAD_MAC, 0, 0), "zeros": (T.NO_TYPE, 0, 0), "long": (T.OK, 23, RR.FULL + 1)}[kind]
        assert len(rec) - 5 <= T.MAX_FRAGMENT


def test_incomplete_last_record_is_no_error():
    st = RR.stream13(_items(), cut=1)
    r = RR.expected_read(st)
    assert (r.records, r.error, r.consumed) == (2, RR.OK, st.offsets[2])
    st7 = RR.stream7905(_items(), cut=5)
    assert RR.expected_read(st7).records == 2
