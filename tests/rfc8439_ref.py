"""RFC 8439 ChaCha20-Poly1305 restated for the tests -- TEST INFRASTRUCTURE ONLY.

The CPU parity checker (oracle/) restates the draft construction and stays as
it is; the RFC side of the message path has this reference instead, tied to two
independent sources: OpenSSL's EVP "ChaCha20-Poly1305" (the stored vectors of
tests/golden/rfc8439_vectors.json, and live where libcrypto loads) and, through
the shared keystream, the draft checker (tests/test_rfc8439_ref.py).

* ``seal`` / ``open`` / ``mac_stream``: RFC 8439 sections 2.3, 2.6 and 2.8 in
  numpy (ChaCha20, vectorised over blocks) and Python integers (Poly1305,
  mac_forge.horner_tag on the padded stream).
* ``decomposed_tags``: the tag as the kernels compute it, tile by tile and
  segment by segment from an exported plan (msg_batch_support.batch_tags on the
  padded stream).
* the shapes and messages the GPU tests and the golden file share, their bytes
  derived with SHAKE-256 so that every machine builds the same ones.
* ``OpenSSL``: EVP_CIPHER_fetch "ChaCha20-Poly1305" through ctypes.

Imports without torch and without a GPU."""
from __future__ import annotations

import ctypes as C
import ctypes.util
import functools
import hashlib
import json
import struct
from pathlib import Path

import numpy as np

import mac_forge as mf
import msg_batch_support as mbs

GOLDEN = Path(__file__).resolve().parent / "golden" / "rfc8439_vectors.json"
TB = mbs.TB  # tile bytes; tests/test_msg_rfc8439_plan.py holds it against the plan
CLAMP = mf.CLAMP
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)


# ---------------------------------------------------------------------------
# the construction
# ---------------------------------------------------------------------------
def chacha20_blocks(key: bytes, nonce12: bytes, counter: int, count: int) -> np.ndarray:
    """Keystream blocks counter .. counter + count - 1 (section 2.3: word 12 the
    32-bit counter, words 13-15 the nonce), as count * 64 bytes."""
    assert len(key) == 32 and len(nonce12) == 12
    if count == 0:
        return np.zeros(0, dtype=np.uint8)
    init = np.empty((16, count), dtype=np.uint32)
    for i, w in enumerate(SIGMA + struct.unpack("<8I", key)):
        init[i] = w
    init[12] = (counter + np.arange(count, dtype=np.uint64)).astype(np.uint32)  # mod 2^32
    for i, w in enumerate(struct.unpack("<3I", nonce12)):
        init[13 + i] = w
    x = init.copy()

    def rotl(v, n):
        return (v << np.uint32(n)) | (v >> np.uint32(32 - n))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 16)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rotl(x[d] ^ x[a], 8)
        x[c] += x[d]; x[b] = rotl(x[b] ^ x[c], 7)

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    x += init
    return np.ascontiguousarray(x.T).astype("<u4").view(np.uint8).reshape(-1)


def poly_key(key: bytes, nonce12: bytes):
    """(r16, s16): the first 32 bytes of block 0 (section 2.6), r not yet clamped."""
    ks = chacha20_blocks(key, nonce12, 0, 1).tobytes()
    return ks[:16], ks[16:32]


def pad16(b: bytes) -> bytes:
    return bytes(-len(b) % 16)


def mac_stream(ad: bytes, ct: bytes) -> bytes:
    """Section 2.8: ad || pad16 || ct || pad16 || le64(|ad|) || le64(|ct|)."""
    return bytes(ad) + pad16(ad) + bytes(ct) + pad16(ct) + struct.pack("<QQ", len(ad), len(ct))


def xor_stream(key: bytes, nonce12: bytes, data: bytes) -> bytes:
    """data XOR keystream blocks 1 onward."""
    n = len(data)
    ks = chacha20_blocks(key, nonce12, 1, (n + 63) // 64)[:n]
    return (np.frombuffer(bytes(data), dtype=np.uint8) ^ ks).tobytes()


def tag_of(key: bytes, nonce12: bytes, ad: bytes, ct: bytes) -> bytes:
    r16, s16 = poly_key(key, nonce12)
    return mf.horner_tag(mac_stream(ad, ct), int.from_bytes(r16, "little") & CLAMP, int.from_bytes(s16, "little"))


def seal(key: bytes, nonce12: bytes, pt: bytes, ad: bytes) -> bytes:
    ct = xor_stream(key, nonce12, pt)
    return ct + tag_of(key, nonce12, ad, ct)


def open(key: bytes, nonce12: bytes, data: bytes, ad: bytes):  # noqa: A001  (the checker's name for it)
    """(rc, plaintext) as oracle.open: 2 and nothing for fewer than 16 bytes; else the
    decryption, which always runs, with rc 0 or 1 (tag mismatch)."""
    if len(data) < 16:
        return 2, b""
    ct, tag = bytes(data[:-16]), bytes(data[-16:])
    return (0 if tag_of(key, nonce12, ad, ct) == tag else 1), xor_stream(key, nonce12, ct)


# ---------------------------------------------------------------------------
# the decomposition the kernels run, from an exported plan
# ---------------------------------------------------------------------------
def single_as_batch(plan: dict) -> dict:
    """msg.plan_for's dict in the form of a one-message batch plan: one segment per group."""
    per, T = plan["tiles_per_group"], plan["tiles"]
    segs = [{"msg": 0, "tile_begin": g * per, "tile_end": min(T, (g + 1) * per), "group": g}
            for g in range(plan["groups"])]
    return {"msgs": [plan], "segs": segs, "msg_segs": [(0, len(segs))]}


def decomposed_tags(msgs, plan: dict, exp_shift: int = 0):
    """The tags of (key, nonce12, ad, ct) messages over a batch plan's tiles and segments."""
    streams = [mac_stream(ad, ct) for _, _, ad, ct in msgs]
    return mbs.batch_tags(streams, [poly_key(k, nc) for k, nc, _, _ in msgs], plan, exp_shift)


# ---------------------------------------------------------------------------
# shapes and messages shared by the GPU tests and the golden file
# ---------------------------------------------------------------------------
KEY = bytes(range(0x40, 0x60))
NONCE = bytes([0xC1, 0x52, 0xE3, 0x74]) + bytes([0xA0, 1, 2, 3, 4, 5, 6, 0x7F])  # nonce_hi: four different bytes
SMALL = (0, 1, 15, 16, 17, 63, 64, 65)
PAD_ADLENS = (0, 1, 13, 15, 16, 17)
EDGE_L = (TB - 16, TB, TB + 16, 2 * TB - 16, 2 * TB, 2 * TB + 16, 3 * TB)
NUM_KEYS = 3
KEYS = b"".join(hashlib.sha256(b"rfc8439 batch key %d" % i).digest() for i in range(NUM_KEYS))


def stream_len(n: int, adlen: int) -> int:
    return -(-adlen // 16) * 16 + -(-n // 16) * 16 + 16


def pad_shapes():
    """Padding and emptiness, as (n, adlen)."""
    return [(n, a) for n in SMALL for a in PAD_ADLENS]


def ad_edge_shapes():
    """The AD's padding at and across a tile edge."""
    return [(n, a) for a in (TB - 17, TB - 16, TB - 15, TB - 1, TB, TB + 1) for n in (0, 1, 100)]


def ct_edge_shapes():
    """adlen 13 (P = 16): the length block last in a tile, alone in one, first behind
    an edge; and one byte shorter, the 15 zeros of padding in front of it."""
    out = []
    for L in EDGE_L:
        n = L - 32
        assert stream_len(n, 13) == L == stream_len(n - 1, 13)
        out += [(n, 13), (n - 1, 13)]
    return out


def single_shapes():
    return pad_shapes() + ad_edge_shapes() + ct_edge_shapes()


def batch_shapes():
    """Forty messages as (adlen, n), msg_batch_support's order: eighteen edge shapes,
    two of 3 TB + 5 bytes, a run of twenty empty ones."""
    edges = [(1, 1), (15, 15), (16, 16), (17, 17), (13, 63), (16, 64), (17, 65),
             (TB - 17, 0), (TB - 16, 1), (TB - 15, 100), (TB, 0), (TB + 1, 100),
             (13, TB - 32), (13, TB - 33), (13, TB - 16), (13, 2 * TB - 32), (13, 2 * TB - 33), (13, 3 * TB - 32)]
    out = edges[:9] + [(13, 3 * TB + 5)] + edges[9:] + [(0, 3 * TB + 5)]
    out += [((0, 1, 13, 16, 17)[i % 5], 0) for i in range(20)]
    assert len(out) == 40
    return out


def data(n: int, what: bytes) -> bytes:
    """n bytes that depend on `what` alone."""
    return hashlib.shake_256(what).digest(n) if n else b""


def single_message(n: int, adlen: int):
    """(key, nonce12, pt, ad) of a shape of the single-message tests."""
    return KEY, NONCE, data(n, b"pt %d %d" % (n, adlen)), data(adlen, b"ad %d %d" % (n, adlen))


def batch_message(i: int, adlen: int, n: int):
    """(key index, nonce12, pt, ad) of message i of a batch: key i % 3, its own nonce."""
    nonce = data(4, b"nonce hi %d" % i) + struct.pack("<Q", 0x0102030405060708 * (i + 1) % 2**64)
    return i % NUM_KEYS, nonce, data(n, b"batch pt %d" % i), data(adlen, b"batch ad %d" % i)


@functools.lru_cache(maxsize=None)
def sealed_single(n: int, adlen: int) -> bytes:
    key, nonce, pt, ad = single_message(n, adlen)
    return seal(key, nonce, pt, ad)


_batch_cache: dict = {}


def batch_messages(shapes=None):
    """msg_batch_support.Msg of every shape, sealed by this reference once."""
    shapes = tuple(batch_shapes() if shapes is None else shapes)
    if shapes not in _batch_cache:
        out = []
        for i, (adlen, n) in enumerate(shapes):
            kidx, nonce, pt, ad = batch_message(i, adlen, n)
            m = mbs.Msg(kidx, nonce, ad, pt, b"", KEYS)
            m.sealed = seal(m.key, nonce, pt, ad)
            out.append(m)
        _batch_cache[shapes] = out
    return _batch_cache[shapes]


def golden() -> dict:
    return json.loads(GOLDEN.read_text())


# ---------------------------------------------------------------------------
# OpenSSL 3: EVP "ChaCha20-Poly1305", IV length 12
# ---------------------------------------------------------------------------
class OpenSSL:
    CTRL_AEAD_SET_IVLEN, CTRL_AEAD_GET_TAG, CTRL_AEAD_SET_TAG = 0x9, 0x10, 0x11

    def __init__(self):
        L = C.CDLL(ctypes.util.find_library("crypto") or "libcrypto.so.3")
        vp, cp, ip = C.c_void_p, C.c_char_p, C.POINTER(C.c_int)
        L.EVP_CIPHER_fetch.restype = vp
        L.EVP_CIPHER_fetch.argtypes = [vp, cp, cp]
        L.EVP_CIPHER_CTX_new.restype = vp
        L.EVP_CIPHER_CTX_free.argtypes = [vp]
        L.EVP_CIPHER_CTX_ctrl.argtypes = [vp, C.c_int, C.c_int, vp]
        for f in (L.EVP_EncryptInit_ex, L.EVP_DecryptInit_ex):
            f.argtypes = [vp, vp, vp, cp, cp]
        for f in (L.EVP_EncryptUpdate, L.EVP_DecryptUpdate):
            f.argtypes = [vp, cp, ip, cp, C.c_int]
        for f in (L.EVP_EncryptFinal_ex, L.EVP_DecryptFinal_ex):
            f.argtypes = [vp, cp, ip]
        L.OpenSSL_version.restype = cp
        L.OpenSSL_version.argtypes = [C.c_int]
        self.L = L
        self.cipher = L.EVP_CIPHER_fetch(None, b"ChaCha20-Poly1305", None)
        if not self.cipher:
            raise OSError("libcrypto has no ChaCha20-Poly1305")
        self.version = L.OpenSSL_version(0).decode()

    def seal(self, key: bytes, nonce12: bytes, pt: bytes, ad: bytes) -> bytes:
        L = self.L
        ctx = L.EVP_CIPHER_CTX_new()
        try:
            assert L.EVP_EncryptInit_ex(ctx, self.cipher, None, None, None) == 1
            assert L.EVP_CIPHER_CTX_ctrl(ctx, self.CTRL_AEAD_SET_IVLEN, 12, None) == 1
            assert L.EVP_EncryptInit_ex(ctx, None, None, key, nonce12) == 1
            ol = C.c_int(0)
            if ad:
                assert L.EVP_EncryptUpdate(ctx, None, C.byref(ol), ad, len(ad)) == 1
            out = C.create_string_buffer(len(pt) + 16)
            if pt:
                assert L.EVP_EncryptUpdate(ctx, out, C.byref(ol), pt, len(pt)) == 1 and ol.value == len(pt)
            fin = C.create_string_buffer(16)
            assert L.EVP_EncryptFinal_ex(ctx, fin, C.byref(ol)) == 1 and ol.value == 0
            tag = C.create_string_buffer(16)
            assert L.EVP_CIPHER_CTX_ctrl(ctx, self.CTRL_AEAD_GET_TAG, 16, tag) == 1
            return out.raw[:len(pt)] + tag.raw
        finally:
            L.EVP_CIPHER_CTX_free(ctx)


def openssl():
    """An OpenSSL, or None where libcrypto or its cipher does not load."""
    try:
        return OpenSSL()
    except (OSError, AttributeError):
        return None
