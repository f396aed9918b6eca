"""Python model of the wave-per-record kernel's Poly1305 (sg_wpr_kernel and
sg_wpr_keying_kernel in suruga_amd/csrc/sg_wpr.hip and sg_wpr_keying.hip) -- TEST
INFRASTRUCTURE ONLY.  tests/test_wpr_mac_model*.py and tests/test_wpr_bucket_model_*.py
hold it against the references, one file per record form; tests/mac_forge.py builds
ciphertext against its T operand.

The record kernel, on the 16 KiB frame (a shorter bucket record lies right-aligned
in it behind i8 zeros, bytes 0x80):

* ciphertext chunk m = 256 j + 128 h + 4 q + i (iteration j, lane 32 h + q,
  chunk i of the lane's 64-byte block) is the i8 B operand (byte - 128) of
  MFMA step (j, i), column q;
* the T operand row c holds the signed base-256 digits of
  V = r^(128 k + 5 - i + delta) for bytes a' < 16 - sigma and of
  P = r^(128 k + 4 - i + delta) otherwise (k = (1 - h) + 2 (3 - j)), read as
  two 16-byte windows of the 48-byte digit lines the kernel builds in LDS
  (V window at 48 iv + 47 - c, P window at 48 iv - 17 - c, iv = 5 k + 4 - i);
* the 32 x 32 accumulator is seeded with 2^24 and must stay a positive 25-bit
  integer;
* lane (hh, q) assembles X = sum_r D[c_r][q] 2^(8 c_r - 32 hh),
  c_r = (r & 3) + 8 (r >> 2) + 4 hh, and multiplies it by
  W = hi[hh][a] lo[b] = 2^(32 hh) R^(8 a + b), R = r^4, 31 - q = 8 a + b.

The keying kernel is one function for every form, and so is keying() here.  From
wpr_geom<C> (geom) it takes the tables and the constant term

    ctot = prefix + suffix + pads + bias - seed

* prefix: the stream bytes in front of the ciphertext (draft: ad || le64(|ad|); RFC
  8439: ad and its zero padding), blocks 0..beta by Horner, times r^m r^(1 + delta);
* suffix: le64(n) at bit 8 sigma of the stream's last two blocks (draft), or the one
  full block le64(|ad|) || le64(n) at weight r (RFC 8439), behind the tail byte's
  block at r^2 where a full TLS 1.3 record has one (its length block says n + 1);
* pads: 2^128 per full block and 2^(8 rem) on the last: 2^128 G(B) + (2^(8 rem) - 2^128) r;
* bias: the 128 the i8 operand takes off every ciphertext byte:
  r^delta G(m) (A1 r + A2), A1 = sum_{k >= sigma} 128 2^(8k), A2 = sum_{k < sigma} 128 2^(8k);
* seed: 2^24 sum_c 2^(8c) SW, SW = sum_{u<32} R^u, what the accumulator started from;
* G(m) = r + .. + r^m and r^m from the table pieces (n = 64 k', k' = 32 a + c, T = r^128):
      S(c)  = sum_{a' < c >> 3} R^(8 a') sum_b R^b + R^(8 (c >> 3)) sum_{b < c & 7} R^b
      S(k') = SW sum_{k < a} T^k + T^a S(c)
      G(m)  = (r + r^2 + r^3 + r^4) S(k'),   r^m = T^a R^(8 (c >> 3)) R^(c & 7)
  At n = 2^14 (a = 8, c = 0) these are the uniform launch's G4 SW sum_k T^k and T^8.

constant_term_by_definition() is the same term from the MAC stream itself and
shares nothing with keying() but P.

Imports without torch and without the native library."""
from __future__ import annotations

import struct
from types import SimpleNamespace

import numpy as np

P = (1 << 130) - 5
C80 = sum(0x80 << (8 * a) for a in range(17))
N = 16384
DRAFT, RFC8439 = "draft", "rfc8439"


def signed_digits(v: int) -> list[int]:
    """The kernel's digit lines: bytes of v + 0x80..80, each minus 0x80."""
    u = v + C80
    d = [((u >> (8 * a)) & 0xFF) ^ 0x80 for a in range(17)]
    return [x - 256 if x >= 128 else x for x in d]


def geo(r: int, m: int) -> int:
    return sum(pow(r, e, P) for e in range(1, m + 1)) % P


def geom(construction: str, adlen: int, n: int, tail: bool = False) -> SimpleNamespace:
    """wpr_geom<C>(adlen, n); tail: the keying kernel's TAIL13 step, one block more behind the m."""
    g = SimpleNamespace(m=n >> 4)
    if construction == RFC8439:
        g.o = -(-adlen // 16) * 16
        g.sigma, g.beta = 0, g.o >> 4
        g.B, g.rem, g.delta = g.beta + g.m + 1, 16, 0
    else:
        g.o = adlen + 8
        g.sigma, g.beta = g.o & 15, g.o >> 4
        L = adlen + 16 + n
        g.B = (L + 15) >> 4
        g.rem = L - 16 * (g.B - 1)
        g.delta = g.B - g.beta - 1 - g.m
    if tail:
        assert construction == RFC8439
        g.B, g.delta = g.B + 1, 1
    assert g.delta in (0, 1)
    return g


def keying(construction: str, ad: bytes, r: int, n: int = N, tail: int | None = None, uniform_sums: bool = False) -> dict:
    """sg_wpr_keying_kernel: the tables and the constant term of one record of n bytes in the
    frame.  tail: ciphertext byte 2^14 of a full TLS 1.3 record.  uniform_sums: G(m) and r^m
    as the uniform launch sums them, right for n = 2^14 only."""
    adlen = len(ad)
    G = geom(construction, adlen, n, tail is not None)
    rdel = pow(r, G.delta, P)
    rd = [pow(r, 1 + G.delta + u, P) for u in range(5)]
    T = pow(r, 128, P)
    tk = [pow(T, k, P) for k in range(8)]
    R = pow(r, 4, P)
    lo = [pow(R, b, P) for b in range(8)]
    hi = [[pow(R, 8 * a, P) * (1 << (32 * h)) % P for a in range(4)] for h in range(2)]
    sw = sum(lo) * sum(hi[0]) % P
    g4 = sum(pow(r, e, P) for e in range(1, 5))
    kq = n >> 6
    ca, cl, ch = kq >> 5, kq & 7, (kq >> 3) & 3
    ta = pow(T, ca, P)
    sc = (hi[0][ch] * sum(lo[:cl]) + sum(hi[0][:ch]) * sum(lo)) % P
    sk = (sw * sum(tk[:ca]) + ta * sc) % P
    g, rm = g4 * sk % P, ta * hi[0][ch] * lo[cl] % P
    if uniform_sums:
        g, rm = g4 * sw * sum(tk) % P, pow(T, 8, P)
    else:
        assert g == geo(r, G.m) and rm == pow(r, G.m, P)
    gb = (g + rm * geo(r, G.B - G.m)) % P
    pads = (1 << 128) * gb + ((1 << (8 * G.rem)) + P - (1 << 128)) * r
    a1 = sum(0x80 << (8 * k) for k in range(G.sigma, 16))
    a2 = sum(0x80 << (8 * k) for k in range(G.sigma))
    bias = g * (a1 * r + a2) * rdel
    cj = (P - ((1 << 24) * sum(1 << (8 * c) for c in range(32))) % P) % P  # sg_wpr_layout.h kCJ*
    seed = cj * sw
    pre = ad + (bytes(G.o - adlen) if construction == RFC8439 else struct.pack("<Q", adlen))
    hp = 0
    for b in range(G.beta + 1):  # (RFC 8439: block beta holds no prefix byte)
        hp = (hp * r + int.from_bytes(pre[16 * b:16 * b + 16], "little")) % P
    prefix = hp * rm * rd[0]
    if tail is not None:
        suffix = tail * r * r + (adlen + ((n + 1) << 64)) * r
    elif construction == RFC8439:
        suffix = (adlen + (n << 64)) * r
    else:
        x = n << (8 * G.sigma)
        suffix = (x % (1 << 128)) * rd[0] + (x >> 128) * rdel
    return dict(sig=G.sigma, rd=rd, tk=tk, lo=lo, hi=hi, ctot=(pads + bias + seed + prefix + suffix) % P)


def constant_term_by_definition(construction: str, ad: bytes, r: int, n: int = N, tail: int | None = None) -> int:
    """ctot from the stream itself: Poly1305's sum (every block with its pad bit) over the
    construction's MAC stream in which every ciphertext byte of the MFMA part is 0x80, the
    i8 operand's zero -- the tail byte keeps its value -- minus what the seeded accumulator
    holds on such a record, 2^24 in each of its 32 x 32 entries."""
    ct = b"\x80" * n + (b"" if tail is None else bytes([tail]))
    if construction == RFC8439:
        stream = ad + bytes(-len(ad) % 16) + ct + bytes(-len(ct) % 16) + struct.pack("<QQ", len(ad), len(ct))
    else:
        stream = ad + struct.pack("<Q", len(ad)) + ct + struct.pack("<Q", len(ct))
    h = 0
    for at in range(0, len(stream), 16):
        block = stream[at:at + 16]
        h = (h + int.from_bytes(block, "little") + (1 << (8 * len(block)))) * r % P
    seeded = (1 << 24) * sum(1 << (8 * c) for c in range(32)) * sum(pow(r, 4 * u, P) for u in range(32))
    return (h - seeded) % P


def digit_lines(kt: dict) -> np.ndarray:
    """The 40 digit lines of 48 bytes in LDS (and the 16 zero bytes read past the last):
    line 5 k + u holds rd[u] tk[k], digit i at byte 47 - sigma - i."""
    lines = np.zeros(40 * 48 + 16, dtype=np.int64)
    for line in range(40):
        k, u = divmod(line, 5)
        d = signed_digits(kt["rd"][u] * kt["tk"][k] % P)
        for i in range(17):
            lines[48 * line + 47 - kt["sig"] - i] = d[i]
    return lines


def t_operand(lines: np.ndarray, sig: int, j: int, i: int, h: int, rows=range(32)):
    """MFMA step (j, i) of half-wave h: the T operand's `rows` (16 digits each) and the 32
    ciphertext chunks, one per column q, they multiply."""
    k = (1 - h) + 2 * (3 - j)
    iv = 5 * k + 4 - i
    T = np.zeros((len(rows), 16), dtype=np.int64)
    for at, c in enumerate(rows):
        vw = lines[48 * iv + 47 - c:48 * iv + 47 - c + 16]
        pw = lines[48 * iv - 17 - c:48 * iv - 17 - c + 16]
        T[at] = np.concatenate([vw[:16 - sig], pw[16 - sig:]])
    return T, 256 * j + 128 * h + 4 * np.arange(32) + i


STEPS = [(j, i, h) for j in range(4) for i in range(4) for h in range(2)]


def frame(ct: bytes) -> bytes:
    """A record right-aligned in the kernel's frame: the bytes before it are i8 zeros."""
    return b"\x80" * (N - len(ct)) + ct


def wpr_tag(ad: bytes, frame: bytes, r: int, s: int, kt: dict) -> bytes:
    """The record kernel on the 16 KiB frame with the keying kernel's record kt (of this ad and r)."""
    assert len(frame) == N
    assert kt["sig"] in (0, (len(ad) + 8) & 15) and kt["rd"][1] == kt["rd"][0] * r % P
    lines = digit_lines(kt)
    chunks = np.frombuffer(frame, dtype=np.uint8).astype(np.int64).reshape(1024, 16) - 128
    D = np.full((32, 32), 1 << 24, dtype=np.int64)  # [c][q]
    for j, i, h in STEPS:
        T, m = t_operand(lines, kt["sig"], j, i, h)
        D += T @ chunks[m].T
    assert D.min() > 0 and D.max() < (1 << 25)
    acc = 0
    for q in range(32):
        a, b = divmod(31 - q, 8)
        for hh in range(2):
            x = sum(int(D[(r_ & 3) + 8 * (r_ >> 2) + 4 * hh, q]) << (8 * (r_ & 3) + 64 * (r_ >> 2)) for r_ in range(16))
            acc += kt["hi"][hh][a] * kt["lo"][b] * x
    acc = (acc + kt["ctot"]) % P
    return ((acc + s) % (1 << 128)).to_bytes(16, "little")
