"""The parallel Poly1305 of the long-message path (suruga_amd/csrc/sg_msg.hip)
restated in Python integers and compared with the oracle's sequential
Poly1305 (poly1305.rs:195-312) on the same MAC stream.

The steps are the kernels': z virtual all-zero blocks (no pad bit) in front of
the stream, each tile's Horner chain h = (h + c) r from h = 0 over its K
blocks, the group fold H_g = H_g R + h_t with R = r^K, the finish
sum_g H_g R^(tiles after group g), and a short last block that carries its pad
bit at its own length.  The geometry comes from sg_msg_plan_for, as it does on
the device.  CPU only."""
from __future__ import annotations

import pytest

from mac_forge import mac_stream
from msg_batch_support import rnd

P1305 = (1 << 130) - 5
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF


def tiled_tag(stream: bytes, r16: bytes, s16: bytes, plan: dict) -> bytes:
    r = int.from_bytes(r16, "little") & CLAMP
    K, T, z, B = plan["tile_blocks"], plan["tiles"], plan["zero_blocks"], plan["mac_blocks"]
    G, per = plan["groups"], plan["tiles_per_group"]
    assert B == (len(stream) + 15) // 16 and z + B == T * K

    def block(v: int) -> int:
        if v < z:
            return 0  # virtual: value 0, no pad bit
        chunk = stream[16 * (v - z):16 * (v - z) + 16]
        return int.from_bytes(chunk, "little") | (1 << (8 * len(chunk)))  # pad bit at the block's own length

    R = pow(r, K, P1305)
    total = 0
    for g in range(G):
        lo, hi = g * per, min(T, (g + 1) * per)
        H = 0
        for t in range(lo, hi):
            h = 0
            for i in range(K):
                h = (h + block(t * K + i)) * r % P1305
            H = (H * R + h) % P1305
        total = (total + H * pow(R, T - hi, P1305)) % P1305
    return ((total + int.from_bytes(s16, "little")) % (1 << 128)).to_bytes(16, "little")


def cases():
    from suruga_amd import msg

    TB = msg.plan_for(0, 0)["tile_bytes"]
    out = []
    # every (adlen + 8) % 16 in {0, 1, 8, 15}; n within +-17 bytes of one, two and three tiles
    for adlen in (8, 9, 0, 7):
        assert (adlen + 8) % 16 in (0, 1, 8, 15)
        for tiles in (1, 2, 3):
            for d in range(-17, 18):
                out.append((adlen, tiles * TB + d))
    # the le64(n) trailer across a tile edge: adlen + 16 + n = 1..7 (mod tile_bytes)
    for adlen in (0, 13):
        for k in (1, 2):
            for m in range(1, 8):
                out.append((adlen, k * TB + m - adlen - 16))
    # AD longer than a tile, and the empty message
    out += [(TB + 5, 0), (2 * TB + 9, 100), (0, 0), (0, 1)]
    return out


def test_tiled_poly1305_equals_the_sequential_one(oracle):
    from suruga_amd import msg

    all_cases = cases()
    data = rnd("stream", max(a + n for a, n in all_cases) + 16)
    for i, (adlen, n) in enumerate(all_cases):
        stream = mac_stream(data[:adlen], data[adlen:adlen + n])
        r16, s16 = rnd(f"r{i}", 16), rnd(f"s{i}", 16)
        want = oracle.poly1305(stream, r16, s16)
        groups = (0, 1, 2, 3)[i % 4]
        assert tiled_tag(stream, r16, s16, msg.plan_for(n, adlen, groups)) == want, (adlen, n, groups)


def test_where_the_trailer_cases_put_le64_n():
    """adlen + 16 + n = 1..7 (mod tile_bytes) is one tile of stream plus 1..7
    bytes: a second tile exists for those bytes alone, and le64(n) lies across
    two MAC blocks, its last 1..7 bytes alone in the short final block.  With
    the virtual zeros in FRONT the stream's end is the last tile's end, so both
    blocks are the last two of the last tile: the trailer cannot cross a tile
    edge in this decomposition, whatever the lengths."""
    from suruga_amd import msg

    TB = msg.plan_for(0, 0)["tile_bytes"]
    for m in range(1, 8):
        n = TB + m - 13 - 16
        p = msg.plan_for(n, 13)
        L = 13 + 16 + n
        assert p["tiles"] == 2 and p["zero_blocks"] == p["tile_blocks"] - 1
        first, last = (L - 8) // 16, (L - 1) // 16  # MAC blocks of the trailer's first and last byte
        assert last == first + 1 == p["mac_blocks"] - 1 and L - 16 * last == m
        assert (p["zero_blocks"] + first) // p["tile_blocks"] == (p["zero_blocks"] + last) // p["tile_blocks"] == 1


def test_model_rejects_a_wrong_decomposition(oracle):
    """The comparison is live: dropping the pad bit of the short last block changes the tag."""
    from suruga_amd import msg

    stream = mac_stream(b"", rnd("x", 21))  # 37 bytes: last block of 5
    r16, s16 = rnd("r", 16), rnd("s", 16)
    want = oracle.poly1305(stream, r16, s16)
    assert tiled_tag(stream, r16, s16, msg.plan_for(21, 0)) == want
    assert tiled_tag(stream + b"\0" * 11, r16, s16, msg.plan_for(21, 0)) != want
