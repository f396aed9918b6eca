"""tests/quic_ref.py against its independent sources: tests/golden/quic_packets.json
(OpenSSL's AEAD and OpenSSL's ChaCha20 for the mask) and RFC 9001 appendix A.5; the packet
number decoding against RFC 9000 appendix A.3's example and its window edges; and
tests/quic_model.py, the kernel's lane decomposition of the MAC, against the sequential tag.
CPU only."""
from __future__ import annotations

import hashlib

import pytest

import mac_forge as mf
import quic_model as QM
import quic_ref as Q
import rfc8439_ref as R


def golden_raw(c):
    """(header || payload with a zeroed packet number field, payload) of a golden case."""
    pn_len = (c["first"] & 3) + 1
    payload = R.data(c["n"], b"quic payload %d" % c["n"])
    return bytes([c["first"]]) + R.data(c["pn_off"] - 1, b"quic header %d" % c["pn_off"]) + bytes(pn_len) + payload, payload


def test_golden_packets():
    g = Q.golden()
    key, iv, hp = (bytes.fromhex(g[k]) for k in ("key", "iv", "hp"))
    assert len(g["cases"]) >= 20
    for c in g["cases"]:
        raw, payload = golden_raw(c)
        pn_len = (c["first"] & 3) + 1
        hdr_len = c["pn_off"] + pn_len
        pkt = Q.protect(key, iv, hp, c["pn"], raw, c["pn_off"])
        assert Q.nonce_of(iv, c["pn"]).hex() == c["nonce"]
        assert pkt[:hdr_len].hex() == c["protected_header"], c
        assert hashlib.sha256(pkt[hdr_len:-16]).hexdigest() == c["ct_sha256"], c
        assert pkt[-16:].hex() == c["tag"], c
        assert Q.hp_mask(hp, bytes.fromhex(c["sample"])).hex() == c["mask"], c
        # ... and back, from an expected number at either edge of the window
        want_hdr = Q.header_of(raw, c["pn_off"], c["pn"])
        half = 1 << (8 * pn_len - 1)
        for exp in {c["pn"], max(0, c["pn"] - half), min(2**62 - 1, c["pn"] + half - 1)}:
            assert Q.unprotect(key, iv, hp, exp, pkt, c["pn_off"]) == (0, want_hdr + payload, c["pn"]), (c, exp)


def test_rfc9001_a5():
    a = Q.A5
    assert Q.packet_keys(a["secret"]) == (a["key"], a["iv"], a["hp"])
    assert Q.next_secret(a["secret"]) == a["ku"]
    raw = a["header"][:1] + bytes(3) + a["payload"]  # the packet number field is the call's to write
    assert Q.header_of(raw, 1, a["pn"]) == a["header"]
    pkt = Q.protect(a["key"], a["iv"], a["hp"], a["pn"], raw, 1)
    assert pkt == a["packet"]
    assert pkt[5:21] == a["sample"] and Q.hp_mask(a["hp"], a["sample"]) == a["mask"]
    for exp in (a["pn"], a["pn"] - 2**23, a["pn"] + 2**23 - 1):
        assert Q.unprotect(a["key"], a["iv"], a["hp"], exp, pkt, 1) == (0, a["header"] + a["payload"], a["pn"])
    assert Q.unprotect(a["key"], a["iv"], a["hp"], a["pn"] + 2**23, pkt, 1)[0] == 1  # outside the window: another nonce


def test_short_packets():
    a = Q.A5
    assert Q.protect(a["key"], a["iv"], a["hp"], 0, b"\x40", 1) is None           # no packet number field
    assert Q.protect(a["key"], a["iv"], a["hp"], 0, b"\x40\x00\x01\x02", 1) is None  # pn_len 1 + 2 payload bytes
    assert len(Q.protect(a["key"], a["iv"], a["hp"], 0, b"\x40\x00\x01\x02\x03", 1)) == 21
    assert Q.unprotect(a["key"], a["iv"], a["hp"], 0, bytes(20), 1) == (2, b"", 0)


def test_decode_pn_a3_example():
    assert Q.decode_pn(0xA82F30EA + 1, 0x9B32, 2) == 0xA82F9B32


@pytest.mark.parametrize("pn_len", (1, 2, 3, 4))
def test_decode_pn_window(pn_len):
    win = 1 << (8 * pn_len)
    half = win // 2
    for exp in (5 * win + 17, 5 * win, 5 * win + win - 1, 2**40 + half):
        # every number of the window (exp - half, exp + half] decodes to itself, both wraps included
        for pn in (exp - half + 1, exp - half + 2, exp - 1, exp, exp + 1, exp + half - 1, exp + half):
            assert Q.decode_pn(exp, pn % win, pn_len) == pn, (exp, pn)
        # one beyond either edge lands a window away
        assert Q.decode_pn(exp, (exp - half) % win, pn_len) == exp + half
        assert Q.decode_pn(exp, (exp + half + 1) % win, pn_len) == exp - half + 1


@pytest.mark.parametrize("pn_len", (1, 2, 3, 4))
def test_decode_pn_ends(pn_len):
    win = 1 << (8 * pn_len)
    half = win // 2
    # expected 0: nothing decodes below zero
    for t in (0, 1, half, half + 1, win - 1):
        assert Q.decode_pn(0, t, pn_len) == t
    # next to 2^62: no candidate is lifted to 2^62 or beyond
    top = 2**62
    for exp in (top - 1, top - half, top - win, top - win - 1):
        for t in (0, 1, half - 1, half, win - 1):
            got = Q.decode_pn(exp, t, pn_len)
            assert got < top and got % win == t, (exp, t, got)
    assert Q.decode_pn(top - 1, 0, pn_len) == top - win
    assert Q.decode_pn(top - win - 1, 0, pn_len) == top - win  # lifted: it stays below 2^62


MODEL_N = (0, 1, 3, 15, 16, 17, 47, 48, 63, 64, 65, 127, 128, 447, 448, 449, 511, 512, 959, 960, 1023, 1024, 1162, 1431,
           2027, 4096, 16107)


@pytest.mark.parametrize("G", (8, 16))
def test_lane_decomposition_is_the_sequential_tag(G):
    key, nonce = R.KEY, R.NONCE
    for n in MODEL_N:
        for adlen in (2, 16, 17, 255):
            ad, ct = R.data(adlen, b"quic model ad %d" % n), R.data(n, b"quic model ct %d" % n)
            assert QM.tag(key, nonce, ad, ct, G) == R.tag_of(key, nonce, ad, ct), (G, n, adlen)


@pytest.mark.parametrize("G", (8, 16))
def test_lane_sets_partition_the_stream(G):
    for n in MODEL_N:
        for adlen in (2, 17, 255):
            sets = QM.lane_sets(adlen, n, G)
            blocks = sorted(b for _, s in sets for b in s)
            assert blocks == list(range(len(R.mac_stream(bytes(adlen), bytes(n))) // 16)), (G, n, adlen)
            nf, q, zc, tail, kt = QM.geom(n, G)
            assert zc >= 1 and G * q - zc == nf and 64 * nf + tail == n and kt == -(-tail // 16)
            assert all(len(s) <= 4 * q + 16 for _, s in sets)


def test_geometry_choice():
    assert QM.lanes_for(2048) == 8 and QM.lanes_for(2049) == 16
    assert mf.P == QM.P
