"""The MAC of sg_quic.hip's kernel in Python integers -- TEST INFRASTRUCTURE ONLY.

The kernel gives a packet G lanes (8 or 16).  With n payload bytes, NF = n // 64 whole
64-byte chunks and a tail of n % 64 bytes, Q = ceil((NF + 1) / G) slots a lane and
zc = G Q - NF >= 1, slot v = t Q + q of lane t holds chunk v - zc (nothing where that is
negative).  A lane's sum H_t is a Horner pass from 0 over the four MAC blocks of each of
its chunks; the additional data's own pass is the value of slot zc - 1 (in front of chunk
0); slot 0 never holds a chunk and takes the tail: TS, a pass from 0 over its kt =
ceil((n % 64) / 16) zero-padded blocks and the length block.  Then

    S = sum_t H_t P^(G - 1 - t),  P = r^(4 Q)     (a Hillis-Steele pass: log2 G steps)
    accumulator = S r^(kt + 1) + TS

``geom`` restates sg_quic.h's Geom, ``lane_sums`` the per-lane values, ``tag`` the whole;
tests/test_quic_ref.py holds ``tag`` against the sequential mac_forge.horner_tag.
``lane_sets`` names each lane's blocks in the MAC stream, for the forged partial sums of
tests/test_gpu_quic.py.  Imports without torch and without a GPU."""
from __future__ import annotations

import mac_forge as mf
import rfc8439_ref as R

P = mf.P
SMALL_MAX = 2048


def lanes_for(max_len: int) -> int:
    return 8 if max_len <= SMALL_MAX else 16


def geom(n: int, G: int):
    """(NF, Q, zc, tail, kt)."""
    nf, tail = n // 64, n % 64
    q = (nf + 1 + G - 1) // G
    return nf, q, G * q - nf, tail, (tail + 15) // 16


def _block(stream: bytes, i: int) -> int:
    return int.from_bytes(stream[16 * i:16 * i + 16], "little") + (1 << 128)


def lane_sets(adlen: int, n: int, G: int):
    """[(lane, blocks)]: the MAC stream blocks (indices into rfc8439_ref.mac_stream) that
    enter lane t's sum H_t, for every lane that has some; the last entry is slot 0's TS
    (lane 0), the tail's blocks and the length block."""
    nf, q, zc, _, kt = geom(n, G)
    na = (adlen + 15) // 16
    out = []
    for t in range(G):
        blocks = []
        for s in range(q):
            v = t * q + s
            if v >= zc:
                blocks += range(na + 4 * (v - zc), na + 4 * (v - zc) + 4)
            if v + 1 == zc:
                blocks += range(na)
        if blocks:
            out.append((t, tuple(blocks)))
    out.append((0, tuple(range(na + 4 * nf, na + 4 * nf + kt + 1))))
    return out


def lane_sums(stream: bytes, adlen: int, n: int, r: int, G: int):
    """(H, TS): the G lane sums and slot 0's."""
    sets = lane_sets(adlen, n, G)
    H = [0] * G

    def horner(blocks):
        h = 0
        for i in blocks:
            h = (h + _block(stream, i)) * r % P
        return h

    for t, blocks in sets[:-1]:
        H[t] = horner(blocks)
    return H, horner(sets[-1][1])


def scan(H, pw: int):
    """The Hillis-Steele pass: after steps 1, 2, 4, ... the last lane holds sum_t H_t pw^(G-1-t)."""
    G, s = len(H), 1
    H = list(H)
    while s < G:
        H = [((H[t - s] if t >= s else 0) * pw + H[t]) % P for t in range(G)]
        pw = pw * pw % P
        s *= 2
    return H[-1]


def tag(key: bytes, nonce12: bytes, ad: bytes, ct: bytes, G: int) -> bytes:
    r16, s16 = R.poly_key(key, nonce12)
    r, s = int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")
    n = len(ct)
    _, q, _, _, kt = geom(n, G)
    H, ts = lane_sums(R.mac_stream(ad, ct), len(ad), n, r, G)
    acc = (scan(H, pow(r, 4 * q, P)) * pow(r, kt + 1, P) + ts) % P
    return ((acc + s) & mf.M128).to_bytes(16, "little")
