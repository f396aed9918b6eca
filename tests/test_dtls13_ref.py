"""tests/dtls13_ref.py against its two fixtures (OpenSSL's records, hashlib's keys), the
lane model of the kernel's MAC (tests/quic_model.py) with a DTLS header as additional data
against the sequential Poly1305, and the sequence number's reconstruction against its
definition at the window's edges.  CPU only."""
from __future__ import annotations

import hashlib

import pytest

import dtls13_ref as D
import mac_forge as mf
import quic_model as QM
import rfc8439_ref as R

EDGE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 8 * 64 - 1, 8 * 64, 8 * 64 + 1, 16 * 64 - 1, 16 * 64, 1431, 2049)


def fixture_record(g, c):
    key, iv, sn = (bytes.fromhex(g[k]) for k in ("key", "iv", "sn_key"))
    cid = R.data(c["cid_len"], b"dtls13 cid %d" % c["cid_len"])
    content = R.data(c["n"], b"dtls13 content %d" % c["n"])
    rec = D.protect(key, iv, sn, c["seq"], content, c["type"], pad_to=c["pad_to"], epoch=c["epoch"], cid=cid,
                    seq16=c["seq16"], length=c["length"])
    return (key, iv, sn), cid, content, rec


def test_fixture_has_the_cases_the_tests_rely_on():
    g = D.golden()
    assert "OpenSSL" in g["source"]
    plain = [c for c in g["cases"] if c["pad_to"] == 0]
    assert {c["n"] for c in plain} == {0, 1, 14, 15, 16, 63, 64, 1431}
    assert {(c["seq16"], c["length"]) for c in plain} == {(a, b) for a in (False, True) for b in (False, True)}
    assert {c["cid_len"] for c in plain} == {0, 1, 11, 12, 250} and {c["seq"] for c in plain} == {0, 2**16 - 1, 2**48 - 1}
    assert len(plain) == 8 * 4 * 5 * 3
    padded = [c for c in g["cases"] if c["pad_to"]]
    assert len(padded) >= 8 and any(c["inner"] == 2**14 + 1 and c["n"] < 2**14 for c in padded)
    assert D.header_len(True, True, 11) == 16 and D.header_len(True, True, 12) == 17


def test_reference_against_the_fixture():
    g = D.golden()
    for k, c in enumerate(g["cases"]):
        (key, iv, sn), cid, content, rec = fixture_record(g, c)
        hl = D.header_len(c["seq16"], c["length"], c["cid_len"])
        assert len(rec) == D.record_len(c["n"], c["pad_to"], c["seq16"], c["length"], c["cid_len"]) == hl + c["inner"] + 16
        assert D.inner_len(c["n"], c["pad_to"]) == c["inner"] and D.nonce_of(iv, c["seq"]).hex() == c["nonce"]
        assert D.sn_mask(sn, rec[hl:hl + 16]).hex() == c["mask"]
        assert (rec[:1] + rec[1 + c["cid_len"]:hl]).hex() == c["protected_header"] and rec[1:1 + c["cid_len"]] == cid
        assert rec[-16:].hex() == c["tag"] and hashlib.sha256(rec[hl:-16]).hexdigest() == c["ct_sha256"]
        # ... and back, the sequence number from its low bits
        for expected in (c["seq"], max(0, c["seq"] - 100), c["seq"] + 100)[:3 if k % 7 == 0 else 1]:
            st, inner, seq, ee, clen, ctype = D.unprotect(lambda ee: (key, iv, sn, expected), rec, c["cid_len"])
            assert (st, seq, ee, clen, ctype) == (D.OK, c["seq"], c["epoch"] % 4, c["n"], c["type"])
            assert inner == D.inner_of(content, c["type"], c["pad_to"])


def test_unprotect_statuses():
    key, iv, sn = R.data(32, b"k"), R.data(12, b"i"), R.data(32, b"s")
    rows = lambda ee: (key, iv, sn, 1000)  # noqa: E731
    cid = b"\x01\x02\x03"
    rec = D.protect(key, iv, sn, 1001, b"hello", 23, cid=cid, seq16=True, length=True, epoch=6)
    assert D.unprotect(rows, rec, 3)[:1] + D.unprotect(rows, rec, 3)[2:] == (D.OK, 1001, 2, 5, 23)
    assert D.unprotect(rows, rec, 3, max_len=len(rec) - 1)[0] == D.SKIPPED
    assert D.unprotect(rows, b"", 3)[0] == D.SHORT and D.unprotect(rows, rec[:8 + 15], 3)[0] == D.SHORT
    for mask in (0x20, 0x40, 0x80, 0x10):
        assert D.unprotect(rows, bytes([rec[0] ^ mask]) + rec[1:], 3)[0] == D.BAD_HEADER
    assert D.unprotect(rows, rec, 0)[0] == D.BAD_HEADER and D.unprotect(rows, rec + b"\x00", 3)[0] == D.BAD_HEADER
    for at in range(len(rec)):
        if at not in (6, 7):  # the length field: BAD_HEADER above
            st = D.unprotect(rows, rec[:at] + bytes([rec[at] ^ 1]) + rec[at + 1:], 3)
            assert st[0] == D.BAD_MAC and st[4:] == (0, 0), at
    for inner in (b"", bytes(1), bytes(40)):
        st = D.unprotect(rows, D.protect_inner(key, iv, sn, 1002, inner, cid=cid), 3)
        assert st == (D.NO_TYPE, inner, 1002, 0, 0, 0)
    assert D.strip(b"abc\x00\x17\x00\x00") == (4, 0x17) and D.strip(b"\x16") == (0, 0x16) and D.strip(b"") is None


def test_keys_against_the_fixture():
    g = D.golden_keys()
    assert g["labels"] == {"key": 32, "iv": 12, "sn": 32, "traffic upd": 32} and "dtls13" in g["source"]
    for c in g["cases"]:
        s = bytes.fromhex(c["secret"])
        assert [x.hex() for x in D.record_keys(s)] == [c["key"], c["iv"], c["sn"]]
        assert D.next_secret(s).hex() == c["traffic upd"]
    s = bytes.fromhex(g["chain"][0]["secret"])
    for gen in g["chain"]:
        assert s.hex() == gen["secret"] and [x.hex() for x in D.record_keys(s)] == [gen["key"], gen["iv"], gen["sn"]]
        s = D.next_secret(s)
    # the label is not TLS 1.3's: same shape, other bytes
    import tls13_keys_ref as H

    assert D.expand_label(bytes(32), b"key", b"", 32) != H.expand_label(bytes(32), b"key", b"", 32)


@pytest.mark.parametrize("G", (8, 16))
@pytest.mark.parametrize("adlen", (2, 16, 17, 255))
def test_lane_model_with_a_header_as_ad(G, adlen):
    """quic_model's sum over lanes, the header's blocks in the slot in front of chunk 0, is
    the sequential Poly1305 of RFC 8439 over the same stream."""
    # the header forms that give these lengths
    seq16, length, cid_len = {2: (False, False, 0), 16: (True, True, 11), 17: (True, True, 12), 255: (True, True, 250)}[adlen]
    key, iv = R.data(32, b"lane key"), R.data(12, b"lane iv")
    for n in EDGE_LENGTHS:
        seq = 2**40 + n
        ad = D.header_of(seq16, length, R.data(cid_len, b"lane cid"), 1, seq, n + 16)
        assert len(ad) == adlen
        nonce, ct = D.nonce_of(iv, seq), R.data(n, b"lane ct %d" % n)
        r16, s16 = R.poly_key(key, nonce)
        want = mf.horner_tag(R.mac_stream(ad, ct), int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little"))
        assert QM.tag(key, nonce, ad, ct, G) == want == R.tag_of(key, nonce, ad, ct), (n, adlen, G)
        # the lane that owns the slot in front of chunk 0 has only empty slots, or slot 0, before it:
        # the kernel takes the header's blocks there first
        nf, q, zc, _, _ = QM.geom(n, G)
        t = (zc - 1) // q
        assert all(v < zc for v in range(t * q, zc - 1))


@pytest.mark.parametrize("nbytes", (1, 2))
def test_sequence_reconstruction_at_the_window_edges(nbytes):
    """decode_seq is sg_quic_decode_pn's arithmetic (tests/quic_ref.py restates it too), and it
    is section 4.2.2's: the number closest to expected with these low bits, in
    (expected - hwin, expected + hwin], and nothing below zero."""
    import quic_ref as Q

    win = 1 << (8 * nbytes)
    h = win // 2
    for expected in (0, 1, h - 1, h, h + 1, win - 1, win, win + 1, 5 * win + 77, 2**16 - 1, 2**16, 2**48 - 1, 2**48, 2**60 + 3):
        for d in (-h - 1, -h, -h + 1, -1, 0, 1, h - 1, h, h + 1):
            s = expected + d
            if s < 0:
                continue
            got = D.decode_seq(expected, s & (win - 1), nbytes)
            assert got == Q.decode_pn(expected, s & (win - 1), nbytes) == D.closest(expected, s & (win - 1), nbytes)
            assert got & (win - 1) == s & (win - 1)
            if -h < d <= h:
                assert got == s, (expected, d)
            elif expected >= win:
                assert got == s + (win if d <= -h else -win), (expected, d)
        for t in range(0, win, max(1, win // 257)):
            got = D.decode_seq(expected, t, nbytes)
            assert got == D.closest(expected, t, nbytes) and got >= 0 and got & (win - 1) == t
