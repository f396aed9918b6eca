"""tests/wg_ref.py against its independent source, tests/golden/wg_packets.json (OpenSSL's
AEAD over a nonce, header and padding built by definition); the order of its checks; the
inner-length rule on hand-built IPv4 and IPv6 headers; and tests/quic_model.py, the
kernel's lane decomposition of the MAC, with the empty AD of a WireGuard message.
CPU only."""
from __future__ import annotations

import hashlib
import struct

import pytest

import quic_model as QM
import rfc8439_ref as R
import wg_ref as W


def test_golden_packets():
    g = W.golden()
    key = bytes.fromhex(g["key"])
    assert len(g["cases"]) == 10 * 4 * 3
    assert {c["n"] for c in g["cases"]} == {0, 1, 15, 16, 17, 63, 64, 65, 1420, 1500}
    assert {c["counter"] for c in g["cases"]} == {0, 2**32 - 1, 2**32, 2**64 - 2**13 - 2}
    assert {c["pad_cap"] for c in g["cases"]} == {0, 1420, 1500}
    for c in g["cases"]:
        inner = R.data(c["n"], b"wg inner %d" % c["n"])
        msg = W.protect(key, c["receiver"], c["counter"], inner, c["pad_cap"])
        assert W.padded_len(c["n"], c["pad_cap"]) == c["padded"] and len(msg) == 32 + c["padded"] == W.message_len(c["n"], c["pad_cap"])
        assert W.nonce_of(c["counter"]).hex() == c["nonce"]
        assert msg[:16].hex() == c["header"], c
        assert hashlib.sha256(msg[16:-16]).hexdigest() == c["ct_sha256"], c
        assert msg[-16:].hex() == c["tag"], c
        st, pt, counter, L = W.unprotect(key, msg, want_inner_len=False)
        assert (st, pt, counter, L) == (0, inner + bytes(c["padded"] - c["n"]), c["counter"], None), c
    assert max(c["counter"] for c in g["cases"]) == W.REJECT_AFTER_MESSAGES - 1


def test_padded_len():
    assert [W.padded_len(n) for n in (0, 1, 15, 16, 17)] == [0, 16, 16, 16, 32]
    # a cap that is no multiple of 16 yields ragged messages; a packet above the cap is not padded
    assert [W.padded_len(n, 1420) for n in (1404, 1409, 1419, 1420, 1421, 1500)] == [1408, 1420, 1420, 1420, 1421, 1500]
    assert [W.padded_len(n, 1500) for n in (1420, 1489, 1497, 1500)] == [1424, 1500, 1500, 1500]
    for cap in (0, 1420, 1500):
        for n in range(0, 1600):
            p = W.padded_len(n, cap)
            assert n <= p < n + 16 and (p % 16 == 0 or p == max(n, cap))


def test_status_order():
    key = R.KEY
    msg = W.protect(key, 7, 9, W.ipv4(20, 20))
    assert W.unprotect(key, msg) == (0, W.ipv4(20, 20) + bytes(12), 9, 20)
    assert W.unprotect(key, msg, max_len=len(msg) - 1)[0] == W.SKIPPED
    assert W.unprotect(key, msg[:31]) == (W.SHORT, None, None, None) and W.unprotect(key, b"") == (W.SHORT, None, None, None)
    # a long, short, wrong-typed message is skipped; a short wrong-typed one is short
    assert W.unprotect(key, b"\x01" + bytes(40), max_len=40)[0] == W.SKIPPED
    assert W.unprotect(key, b"\x01" + bytes(30))[0] == W.SHORT
    for typ in (b"\x01\0\0\0", b"\x04\0\0\x01", b"\x04\x01\0\0", b"\0\0\0\x04"):
        assert W.unprotect(key, typ + msg[4:]) == (W.BAD_HEADER, None, None, None)
    # the receiver index is not authenticated and not read; the counter is the nonce
    assert W.unprotect(key, msg[:4] + b"\xff\xff\xff\xff" + msg[8:])[0] == 0
    bad = bytearray(msg)
    bad[8] ^= 1
    st, pt, counter, L = W.unprotect(key, bytes(bad))
    assert (st, counter, L) == (W.BAD_MAC, 8, 0) and len(pt) == 32
    bad = bytearray(msg)
    bad[-1] ^= 0x80
    assert W.unprotect(key, bytes(bad)) == (W.BAD_MAC, W.ipv4(20, 20) + bytes(12), 9, 0)
    # a keepalive
    ka = W.protect(key, 1, 2**40, b"")
    assert len(ka) == 32 and W.unprotect(key, ka) == (0, b"", 2**40, 0) and W.unprotect(key, ka, False) == (0, b"", 2**40, None)


@pytest.mark.parametrize("n", (20, 21, 40, 48, 1424))
def test_inner_length_ipv4(n):
    for L, ok in ((19, False), (20, True), (n, True), (n + 1, False), (0, False), (0xFFFF, False)):
        assert W.inner_len_of(W.ipv4(L, n)) == (L if ok else None), (n, L)
    # the version nibble alone decides; the header length nibble is not looked at
    pkt = bytearray(W.ipv4(20, n))
    pkt[0] = 0x4F
    assert W.inner_len_of(bytes(pkt)) == 20
    pkt[0] = 0x55  # version 5
    assert W.inner_len_of(bytes(pkt)) is None
    assert W.inner_len_of(W.ipv4(19, 19)) is None and W.inner_len_of(W.ipv4(1, 1)) is None  # no room for a header


@pytest.mark.parametrize("n", (40, 41, 55, 1440))
def test_inner_length_ipv6(n):
    for pl, ok in ((0, True), (n - 40, True), (n - 39, False), (0xFFFF, False)):
        assert W.inner_len_of(W.ipv6(pl, n)) == (40 + pl if ok else None), (n, pl)
    assert W.inner_len_of(W.ipv6(0, 39)) is None  # an IPv6 header in 39 bytes
    assert W.inner_len_of(W.ipv6(0, 20)) is None


def test_inner_length_through_unprotect():
    key = R.KEY
    for inner, pad in ((W.ipv4(20, 20), 12), (W.ipv4(33, 33), 15), (W.ipv6(8, 48), 0), (W.ipv6(9, 49), 15)):
        msg = W.protect(key, 3, 5, inner)
        assert len(msg) == 32 + len(inner) + pad
        assert W.unprotect(key, msg) == (0, inner + bytes(pad), 5, len(inner))
    for inner in (W.ipv4(19, 32), W.ipv4(33, 32), W.ipv6(9, 48), bytes([0x55]) + bytes(47), bytes(16), W.ipv4(16, 16)):
        msg = W.protect(key, 3, 6, inner)
        assert W.unprotect(key, msg) == (W.BAD_INNER, inner, 6, 0)
        assert W.unprotect(key, msg, want_inner_len=False) == (0, inner, 6, None)


def test_header_and_nonce_layout():
    assert W.header_of(0x11223344, 0x0102030405060708) == bytes.fromhex("04000000" "44332211" "0807060504030201")
    assert W.nonce_of(0x0102030405060708) == bytes(4) + struct.pack("<Q", 0x0102030405060708)


WG_MODEL_N = (0, 16, 32, 48, 64, 80, 448, 512, 1424, 1504, 16352, 1, 17, 63, 65, 1420)


@pytest.mark.parametrize("G", (8, 16))
def test_lane_decomposition_with_an_empty_ad(G):
    """The kernel's MAC is quic_model's with adlen = 0: the slot in front of chunk 0 holds nothing."""
    key, nonce = R.KEY, W.nonce_of(2**32)
    for n in WG_MODEL_N:
        ct = R.data(n, b"wg model ct %d" % n)
        assert QM.tag(key, nonce, b"", ct, G) == R.tag_of(key, nonce, b"", ct), (G, n)
        blocks = sorted(b for _, s in QM.lane_sets(0, n, G) for b in s)
        assert blocks == list(range(len(R.mac_stream(b"", bytes(n))) // 16)), (G, n)
