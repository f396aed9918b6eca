"""What the TLS 1.3 record-batch GPU tests share -- TEST INFRASTRUCTURE ONLY.

Whole-buffer runs in the way of tests/rfc_batch_support.py: every device buffer
starts as footprint.sentinel with a margin in front and behind and is compared whole
afterwards, so a stray write fails as a wrong byte does -- the record's n + 17 bytes
and nothing from byte n + 17 on; the status, inner_type and content_len arrays
likewise, with a sentinel tail behind their `count` entries.

The reference is tests/tls13_ref.py.  Records take key, IV and sequence number by
index: keys and IVs are rfc_batch_support's three.

Imports without torch and without a GPU."""
from __future__ import annotations

import numpy as np

import footprint as fp
import rfc8439_ref as R
import rfc_batch_support as S
import tls13_ref as T
from gpu_support import slots

M = fp.MARGIN
P = S.P
KEYS3, IVS3 = S.KEYS3, S.IVS3
N = 1 << 14


def key_iv(k: int, ivs: bytes = IVS3, keys: bytes = KEYS3):
    return keys[32 * k:32 * k + 32], ivs[12 * k:12 * k + 12]


class Tls13Case(S.RfcCase):
    """gpu_support.BatchCase through sg_*_batch_tls13: TLS mode, key, IV and sequence
    number by index; the layout alone (the records' bytes are the caller's)."""

    def common(self, ads_h=None) -> dict:
        c = super().common(ads_h)
        del c["rfc8439"]
        return c


def _case(lens, tail, kidx, seqs, skew, strides, ivs, keys, ctype=23):
    """(case, input bytes, output bytes) of a seal of records of `lens` bytes that grow
    by `tail`: back-to-back slots of 16 bytes plus skew, or strides = (in, out)."""
    kw = dict(kidx=np.asarray(kidx, dtype=np.uint32), seqs=np.asarray(seqs, dtype=np.uint64), ivs_h=ivs, content_type=ctype,
              version=(3, 3), tail=tail)
    if strides is not None:
        return Tls13Case(lens, None, keys, strides=tuple(strides), **kw), strides[0] * len(lens), strides[1] * len(lens)
    in_off, out_off, in_size, out_size = slots(lens, 16, skew, tail)
    return Tls13Case(lens, None, keys, in_off=in_off, out_off=out_off, **kw), in_size, out_size


def expected_sealed(contents, kidx, seqs, ctype=23, ivs=IVS3, keys=KEYS3):
    return [T.seal(*key_iv(int(k), ivs, keys), int(q), c, ctype) for c, k, q in zip(contents, kidx, seqs)]


def _check_route(batch, open_: bool, route):
    from suruga_amd import batch as B

    if route is not None:
        assert B.tls13_route(batch, open_) == route, ("route", "open" if open_ else "seal", route)


def seal_whole(contents, kidx, seqs, *, ctype=23, skew=(0, 0), strides=None, want=None, ivs=IVS3, keys=KEYS3, route=None,
               where=()):
    """sg_seal_batch_tls13 into a sentinel buffer with margins: the whole output must be
    the sentinel with every record's reference fragment (len + 17 bytes) laid over it and
    the input unchanged.  Returns the fragments as the device wrote them.  route: what
    sg_batch_tls13_route must say of this very batch."""
    from suruga_amd import batch as B

    lens = [len(c) for c in contents]
    case, in_size, out_size = _case(lens, 17, kidx, seqs, skew, strides, ivs, keys, ctype)
    want = expected_sealed(contents, kidx, seqs, ctype, ivs, keys) if want is None else want
    in_img = np.concatenate([fp.sentinel(M, 0x31), fp.image(max(in_size, 1), 0x77, zip(case.in_off, contents)),
                             fp.sentinel(M, 0x32)])
    size = M + fp.round_up(out_size, 16) + M
    rs = [(M + lo, M + hi) for lo, hi in map(case.out_range, range(case.count))]

    def call(d):
        batch = B.Batch(inp=d["inp"][M:], out=d["out"][M:], **case.seal_args(max(max(lens), 1)))
        _check_route(batch, False, route)
        B.seal_tls13(batch)

    o = fp.run_whole(call, in_img, fp.sentinel(size, 0x5A), fp.image(size, 0x5A, [(lo, w) for (lo, _), w in zip(rs, want)]), rs)
    o.check(where=(*where, "seal"))
    return [o.out[lo:hi].tobytes() for lo, hi in rs]


def open_whole(frags, kidx, seqs, *, skew=(0, 0), strides=None, keep=False, ivs=IVS3, keys=KEYS3, route=None, where=()):
    """sg_open_batch_tls13 of the fragments into sentinel buffers, against the reference's
    open under the same keys, IVs and sequence numbers (which may be wrong ones: then the
    reference says so).  Per record the whole output is its inner plaintext (status 0 and
    5), exactly len - 16 zero bytes (status 1; with keep the decryption) or nothing (status
    2); status, inner_type and content_len are the reference's, and every byte behind them
    is untouched.  Returns the (status, type, content_len) triples; strides = (fragment
    stride, output stride)."""
    from suruga_amd import batch as B

    count = len(frags)
    flens = np.array([len(f) for f in frags], dtype=np.uint32)
    inner = [max(int(n) - 16, 0) for n in flens]
    # the layout of a seal of the inner plaintexts, run backwards
    case, out_size, in_size = _case(inner, 16, kidx, seqs, skew, strides and strides[::-1], ivs, keys)
    exp = [T.open(*key_iv(int(k), ivs, keys), int(q), f) for f, k, q in zip(frags, kidx, seqs)]
    parts = []
    for o, (st, plain, _, _) in zip(case.in_off, exp):
        if st in (T.OK, T.NO_TYPE) or (st == T.BAD_MAC and keep):
            parts.append((M + int(o), plain))
        elif st == T.BAD_MAC:
            parts.append((M + int(o), bytes(len(plain))))
    in_img = np.concatenate([fp.sentinel(M, 0x33), fp.image(max(in_size, 1), 0x78, zip(case.out_off, frags)),
                             fp.sentinel(M, 0x34)])
    size = M + fp.round_up(max(out_size, 1), 16) + M
    rs = [(M + int(o), M + int(o) + n) for o, n in zip(case.in_off, inner)]

    def call(d):
        batch = B.Batch(inp=d["inp"][M:], out=d["out"][M:], status=d["status"], inner_type=d["inner_type"],
                        content_len=d["content_len"], keep_failed=keep, **case.open_args(flens, max(int(flens.max()), 1)))
        _check_route(batch, True, route)
        B.open_tls13(batch)

    o = fp.run_whole(call, in_img, fp.sentinel(size, 0xA5), fp.image(size, 0xA5, parts), rs,
                     arrays={"status": fp.array_start(count, 0x51), "inner_type": fp.array_start(count, 0x52),
                             "content_len": fp.array_start(count, 0x53, np.uint32)})
    want = [(s, t, c) for s, _, t, c in exp]
    o.check(*zip(*want), where=(*where, "open"))
    return want


# ---------------------------------------------------------------------------
# forged accumulators for the TLS 1.3 stream
# ---------------------------------------------------------------------------
def forge_content(k: int, seq: int, n: int, target: int, seed: str, ctype: int = 23):
    """n content bytes (n >= 32) whose sealed record's Poly1305 accumulator is == target
    (mod p) before s is added -- rfc_batch_support.forge_ct's method on the inner
    ciphertext of n + 1 bytes: its last byte is what the type byte encrypts to, its first
    block is solved for, the rest is redrawn until that block lies below 2^128."""
    assert n >= 32
    key, iv = key_iv(k)
    nonce, ad = T.nonce(iv, seq), T.header(n + 17)
    tail = R.xor_stream(key, nonce, bytes(n) + bytes([ctype]))[n]
    r16, _ = R.poly_key(key, nonce)
    r = int.from_bytes(r16, "little") & R.CLAMP
    for t in range(200):
        ct = bytearray(S.rnd(n, f"forge13 {seed} {t}") + bytes([tail]))
        ct[:16] = bytes(16)
        stream = R.mac_stream(ad, bytes(ct))
        nb = len(stream) // 16
        h = 0
        for j in range(nb):
            h = (h + int.from_bytes(stream[16 * j:16 * j + 16], "little") + (1 << 128)) * r % P
        c = (target - h) * pow(pow(r, nb - 1, P), -1, P) % P  # ciphertext block 0 is stream block 1 (one AD block)
        if c < (1 << 128):
            ct[:16] = c.to_bytes(16, "little")
            assert S.accumulator(key, nonce, ad, bytes(ct)) == target % P
            return R.xor_stream(key, nonce, bytes(ct))[:n]
    raise AssertionError("no forgery in 200 tries")
