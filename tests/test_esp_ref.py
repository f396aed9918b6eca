"""tests/esp_ref.py against its independent source, tests/golden/esp_packets.json (OpenSSL's
AEAD over a header, nonce, additional data and trailer built by definition); the order of
its checks; the trailer rule; seq_hi (RFC 4303 appendix A2.1 as Linux writes it) against
the interval definition; and tests/quic_model.py, the kernel's lane decomposition of the
MAC, with the 8- and 12-byte AD of an ESP packet.  CPU only."""
from __future__ import annotations

import hashlib
import random
import struct

import pytest

import esp_ref as E
import quic_model as QM
import rfc8439_ref as R


def test_golden_packets():
    g = E.golden()
    cases = g["cases"][:-1]
    assert len(cases) == 9 * 3 * 2 * 4 * 2
    assert {c["n"] for c in cases} == {0, 1, 2, 61, 62, 63, 64, 1400, 1438}
    assert {c["align"] for c in cases} == {4, 16, 256} and {c["esn"] for c in cases} == {False, True}
    assert {c["seq"] for c in cases} == {0, 2**32 - 1, 2**32, 2**64 - 1}
    assert {c["iv"] is None for c in cases} == {False, True}
    assert {c["padded"] - c["n"] - 2 for c in cases} >= {0, 1, 2, 3, 13, 14, 254}
    for c in g["cases"]:
        key, salt = bytes.fromhex(c.get("key", g["key"])), bytes.fromhex(c.get("salt", g["salt"]))
        payload = bytes.fromhex(c["payload"]) if "payload" in c else R.data(c["n"], b"esp payload %d" % c["n"])
        kw = dict(align=c["align"], esn=c["esn"], iv=c["iv"])
        pkt = E.protect(key, salt, c["spi"], c["seq"], payload, c["next_header"], **kw)
        assert E.padded_len(c["n"], c["align"]) == c["padded"] and len(pkt) == 32 + c["padded"] == E.packet_len(c["n"], c["align"])
        seq = c["seq"] if c["esn"] else c["seq"] & E.M32
        iv = seq if c["iv"] is None else c["iv"]
        assert E.nonce_of(salt, iv).hex() == c["nonce"] and E.ad_of(c["spi"], seq, c["esn"]).hex() == c["ad"]
        assert len(c["ad"]) == (24 if c["esn"] else 16)
        assert pkt[:16].hex() == c["header"], c
        assert hashlib.sha256(pkt[16:-16]).hexdigest() == c["ct_sha256"], c
        assert pkt[-16:].hex() == c["icv"], c
        # the receiver's window ends at the packet: the inferred high half is the sealed one
        got = E.unprotect(key, salt, c["spi"], pkt, esn=c["esn"], top=seq, window=64)
        pad = c["padded"] - c["n"] - 2
        assert got == (0, payload + E.trailer(pad, c["next_header"]), seq, c["n"], c["next_header"]), c


def test_rfc7634_appendix_a_structure():
    c = E.golden()["cases"][-1]
    assert (c["key"], c["salt"], c["spi"], c["seq"], c["iv"]) == (bytes(range(0x80, 0xA0)).hex(), "a0a1a2a3", 0x01020304, 5,
                                                                   0x1011121314151617)
    assert (c["n"], c["next_header"], c["align"], c["esn"], c["padded"]) == (84, 4, 4, False, 88)
    assert c["header"] == "01020304" "00000005" "1011121314151617"
    assert c["nonce"] == "a0a1a2a3" "1011121314151617" and c["ad"] == "01020304" "00000005"
    assert E.trailer(E.pad_len(84), 4) == bytes.fromhex("01020204")


def test_padded_len():
    assert [E.padded_len(n) for n in (0, 1, 2, 3, 6, 7)] == [4, 4, 4, 8, 8, 12]
    assert [E.pad_len(n, 256) for n in (0, 1, 253, 254, 255)] == [254, 253, 1, 0, 255]
    for align in range(4, 257, 4):
        for n in range(0, 600):
            p = E.padded_len(n, align)
            assert p % align == 0 and n + 2 <= p < n + 2 + align and E.pad_len(n, align) == p - n - 2 <= 255
    assert E.packet_len(16350, 4) == E.packet_len(16350, 16) == E.MAX_PACKET_LEN


def test_status_order_and_failures():
    key, salt, spi = R.KEY, b"\x01\x02\x03\x04", 0xC0FFEE01
    payload = R.data(20, b"esp order")
    pkt = E.protect(key, salt, spi, 9, payload, 41)
    assert len(pkt) == 56 and E.unprotect(key, salt, spi, pkt) == (0, payload + b"\x01\x02\x02\x29", 9, 20, 41)
    assert E.unprotect(key, salt, spi, pkt, max_len=len(pkt) - 1)[0] == E.SKIPPED
    assert E.unprotect(key, salt, spi, pkt[:33]) == (E.SHORT, None, None, None, None)
    assert E.unprotect(key, salt, spi, b"") == (E.SHORT, None, None, None, None)
    # a long, wrong-SPI packet is skipped; a short wrong-SPI one is short
    assert E.unprotect(key, salt, spi + 1, pkt, max_len=40)[0] == E.SKIPPED
    assert E.unprotect(key, salt, spi + 1, pkt[:20])[0] == E.SHORT
    assert E.unprotect(key, salt, spi + 1, pkt) == (E.BAD_HEADER, None, None, None, None)
    assert E.unprotect(key, salt, spi ^ 0x80000000, pkt) == (E.BAD_HEADER, None, None, None, None)
    for at in (4, 7, 8, 15, 16, 30, 39, 40, 55):
        bad = bytearray(pkt)
        bad[at] ^= 0x10
        st, pt, seq, n, nh = E.unprotect(key, salt, spi, bytes(bad))
        assert (st, n, nh) == (E.BAD_MAC, 0, 0) and len(pt) == 24 and (seq == 9) == (at >= 8), at
    assert E.unprotect(key, salt, spi, pkt, want_trailer=False) == (0, payload + b"\x01\x02\x02\x29", 9, None, None)
    # ESN: the high half is not on the wire; a window one subspace off fails the ICV with no wire bit changed
    pkt = E.protect(key, salt, spi, 5 * 2**32 + 7, payload, 4, esn=True)
    assert pkt[4:8] == bytes([0, 0, 0, 7])
    assert E.unprotect(key, salt, spi, pkt, esn=True, top=5 * 2**32 + 100, window=128)[:3:2] == (0, 5 * 2**32 + 7)
    st, _, seq, _, _ = E.unprotect(key, salt, spi, pkt, esn=True, top=6 * 2**32 + 100, window=128)
    assert (st, seq) == (E.BAD_MAC, 6 * 2**32 + 7)
    # without ESN the high half of the sequence number is ignored, also as the IV
    assert E.protect(key, salt, spi, 5 * 2**32 + 7, payload, 4) == E.protect(key, salt, spi, 7, payload, 4)


def test_trailer_rule():
    key, salt, spi = R.KEY, b"\xa0\xa1\xa2\xa3", 7
    body = R.data(40, b"esp trailer")

    def through(pt):
        return E.unprotect(key, salt, spi, E.protect_plain(key, salt, spi, 3, pt))

    assert through(body + b"\x01\x02\x03\x03\x32") == (0, body + b"\x01\x02\x03\x03\x32", 3, 40, 0x32)
    assert through(body + b"\x00\x04") == (0, body + b"\x00\x04", 3, 40, 4)
    for wrong in (b"\x00\x02\x03\x03\x04", b"\x01\x03\x03\x03\x04", b"\x01\x02\x04\x03\x04", b"\x02\x03\x04\x03\x04"):
        assert through(body + wrong) == (E.BAD_INNER, body + wrong, 3, 0, 0)
    # pad + 2 == n: all padding, an empty payload; pad + 2 == n + 1: one more than fits
    all_pad = bytes(range(1, 11)) + b"\x0a\x3b"
    assert through(all_pad) == (0, all_pad, 3, 0, 59)
    assert through(bytes(range(2, 11)) + b"\x0a\x3b")[0] == E.BAD_INNER
    assert through(b"\xff\x04")[0] == E.BAD_INNER and through(b"\x00\x04") == (0, b"\x00\x04", 3, 0, 4)
    assert E.parse_trailer(bytes(range(1, 256)) + b"\xff\x04") == (0, 4)


def test_seq_hi_against_the_interval():
    """xfrm_replay_seqhi's two cases give the one number with these low bits in
    [T - W + 1, T - W + 1 + 2^32), mod 2^64."""
    rng = random.Random(4303)
    seen = set()

    def check(top, w, lo):
        want = E.seq_in_window(top, w, lo)
        assert want & E.M32 == lo and E.seq_hi(top, w, lo) == want >> 32, (hex(top), w, hex(lo))
        seen.add((top & E.M32) >= w - 1)

    for _ in range(20000):
        w = rng.choice((1, 2, 32, 64, 1024, 2**31, rng.randrange(1, 2**31 + 1)))
        tl = rng.choice((rng.randrange(2**32), (w - 2) & E.M32, w - 1, 2**32 - 1, 0, w))
        top = rng.choice((0, 1, rng.randrange(2**32), 2**32 - 1)) << 32 | (tl & E.M32)
        bl = (tl - w + 1) & E.M32
        for lo in (rng.randrange(2**32), (bl - 1) & E.M32, bl, (bl + 1) & E.M32, tl & E.M32, 0, 2**32 - 1):
            check(top, w, lo)
    assert seen == {False, True}  # both cases of the appendix
    # Th = 0 with the window over the start: the guess wraps, and fails its ICV
    assert E.seq_hi(5, 64, 2**32 - 10) == 2**32 - 1 and E.seq_in_window(5, 64, 2**32 - 10) == 2**64 - 10
    for w in (1, 64, 2**31):
        for tl in ((w - 2) & E.M32, w - 1, 2**32 - 1):
            top = 7 << 32 | tl
            assert E.seq_hi(top, w, tl) == 7  # the top itself
            assert E.seq_hi(top, w, (tl + 1) & E.M32) == (8 if tl == 2**32 - 1 else 7)
            assert E.seq_in_window(top, w, (tl - w + 1) & E.M32) == top - w + 1


def test_header_nonce_and_ad_layout():
    assert E.header_of(0x11223344, 0x0102030405060708, 0xA1A2A3A4A5A6A7A8) == bytes.fromhex("11223344" "05060708" "a1a2a3a4a5a6a7a8")
    assert E.nonce_of(b"\x09\x08\x07\x06", 0x0102030405060708) == b"\x09\x08\x07\x06" + struct.pack(">Q", 0x0102030405060708)
    assert E.ad_of(0x11223344, 0x0102030405060708, False) == bytes.fromhex("11223344" "05060708")
    assert E.ad_of(0x11223344, 0x0102030405060708, True) == bytes.fromhex("11223344" "01020304" "05060708")


ESP_MODEL_N = (2, 4, 16, 60, 64, 68, 448, 512, 1440, 16352, 3, 17, 63, 65, 255, 257)


@pytest.mark.parametrize("G", (8, 16))
@pytest.mark.parametrize("adlen", (8, 12))
def test_lane_decomposition_with_the_esp_ad(G, adlen):
    """The kernel's MAC is quic_model's with one block of AD in the slot in front of chunk 0."""
    key, nonce, ad = R.KEY, E.nonce_of(b"salt", 2**32), E.ad_of(0xDEADBEEF, 2**40 + 5, adlen == 12)
    assert len(ad) == adlen
    for n in ESP_MODEL_N:
        ct = R.data(n, b"esp model ct %d" % n)
        assert QM.tag(key, nonce, ad, ct, G) == R.tag_of(key, nonce, ad, ct), (G, n)
        blocks = sorted(b for _, s in QM.lane_sets(adlen, n, G) for b in s)
        assert blocks == list(range(len(R.mac_stream(ad, bytes(n))) // 16)), (G, n)
