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
from gpu_support import dev_bytes, dev_u8, dev_u32, dev_u64, host_np

M = fp.MARGIN
PAD = 64          # sentinel entries behind the per-record output arrays
P = S.P
KEYS3, IVS3 = S.KEYS3, S.IVS3
N = 1 << 14


def key_iv(k: int, ivs: bytes = IVS3, keys: bytes = KEYS3):
    return keys[32 * k:32 * k + 32], ivs[12 * k:12 * k + 12]


def slots(lens, skew: int):
    """Back-to-back slots of the lengths rounded up to 16, plus skew bytes: offsets, size."""
    lens = np.asarray(lens, dtype=np.uint64)
    step = (lens + 15) // 16 * 16 + skew
    off = np.zeros(len(lens), dtype=np.uint64)
    off[1:] = np.cumsum(step[:-1])
    return off, int(off[-1] + step[-1])


def _layout(in_lens, out_lens, skew, strides):
    """(in_off, in_size, out_off, out_size); strides = (in_stride, out_stride) for a uniform batch."""
    count = len(in_lens)
    if strides is not None:
        assert len(set(in_lens)) == 1
        idx = np.arange(count, dtype=np.uint64)
        return idx * strides[0], strides[0] * count, idx * strides[1], strides[1] * count
    in_off, in_size = slots(in_lens, skew[0])
    out_off, out_size = slots(out_lens, skew[1])
    return in_off, in_size, out_off, out_size


def _common(count, kidx, seqs, ivs, keys):
    return dict(count=count, keys=dev_bytes(keys).view(3, 32), ivs=dev_bytes(ivs).view(3, 12),
                key_index=dev_u32(np.asarray(kidx, dtype=np.uint32)), seq=dev_u64(np.asarray(seqs, dtype=np.uint64)))


def _shape(lens, in_off, out_off, strides):
    if strides is not None:
        return dict(uniform_len=int(lens[0]), in_stride=strides[0], out_stride=strides[1])
    return dict(lens=dev_u32(np.asarray(lens, dtype=np.uint32)), max_len=max(int(max(lens)), 1), in_off=dev_u64(in_off),
                out_off=dev_u64(out_off))


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
    import torch

    from suruga_amd import batch as B

    count = len(contents)
    lens = [len(c) for c in contents]
    in_off, in_size, out_off, out_size = _layout(lens, [n + 17 for n in lens], skew, strides)
    want = expected_sealed(contents, kidx, seqs, ctype, ivs, keys) if want is None else want
    in_img = np.concatenate([fp.sentinel(M, 0x31), fp.image(max(in_size, 1), 0x77, [(int(o), c) for o, c in zip(in_off, contents)]),
                             fp.sentinel(M, 0x32)])
    size = M + fp.round_up(out_size, 16) + M
    want_img = fp.image(size, 0x5A, [(M + int(o), w) for o, w in zip(out_off, want)])
    d_in, d_out = dev_u8(in_img), dev_u8(fp.sentinel(size, 0x5A))
    batch = B.Batch(inp=d_in[M:], out=d_out[M:], content_type=ctype, **_common(count, kidx, seqs, ivs, keys),
                    **_shape(lens, in_off, out_off, strides))
    _check_route(batch, False, route)
    B.seal_tls13(batch)
    torch.cuda.synchronize()
    got = host_np(d_out)
    rs = [(M + int(o), M + int(o) + n + 17) for o, n in zip(out_off, lens)]
    assert (d := fp.first_diff(got, want_img, rs)) is None, (*where, "seal output", d)
    assert (d := fp.first_diff(host_np(d_in), in_img)) is None, (*where, "seal input changed", d)
    return [got[lo:hi].tobytes() for lo, hi in rs]


def open_whole(frags, kidx, seqs, *, skew=(0, 0), strides=None, keep=False, ivs=IVS3, keys=KEYS3, route=None, where=()):
    """sg_open_batch_tls13 of the fragments into sentinel buffers, against the reference's
    open under the same keys, IVs and sequence numbers (which may be wrong ones: then the
    reference says so).  Per record the whole output is its inner plaintext (status 0 and
    5), exactly len - 16 zero bytes (status 1; with keep the decryption) or nothing (status
    2); status, inner_type and content_len are the reference's, and every byte behind them
    is untouched.  Returns the (status, type, content_len) triples; strides = (fragment
    stride, output stride)."""
    import torch

    from suruga_amd import batch as B

    count = len(frags)
    lens = [len(f) for f in frags]
    in_off, in_size, out_off, out_size = _layout(lens, [max(n - 16, 0) for n in lens], (skew[1], skew[0]), strides)
    exp = [T.open(*key_iv(int(k), ivs, keys), int(q), f) for f, k, q in zip(frags, kidx, seqs)]
    parts = []
    for o, (st, inner, _, _) in zip(out_off, exp):
        if st in (T.OK, T.NO_TYPE) or (st == T.BAD_MAC and keep):
            parts.append((M + int(o), inner))
        elif st == T.BAD_MAC:
            parts.append((M + int(o), bytes(len(inner))))
    in_img = np.concatenate([fp.sentinel(M, 0x33), fp.image(max(in_size, 1), 0x78, [(int(o), f) for o, f in zip(in_off, frags)]),
                             fp.sentinel(M, 0x34)])
    size = M + fp.round_up(max(out_size, 1), 16) + M
    want_img = fp.image(size, 0xA5, parts)
    d_in, d_out = dev_u8(in_img), dev_u8(fp.sentinel(size, 0xA5))
    d_st, d_ty = dev_u8(fp.sentinel(count + PAD, 0x51)), dev_u8(fp.sentinel(count + PAD, 0x52))
    cl0 = fp.sentinel(4 * (count + PAD), 0x53).view(np.uint32)
    d_cl = dev_u32(cl0)
    batch = B.Batch(inp=d_in[M:], out=d_out[M:], status=d_st, inner_type=d_ty, content_len=d_cl, keep_failed=keep,
                    **_common(count, kidx, seqs, ivs, keys), **_shape(lens, in_off, out_off, strides))
    _check_route(batch, True, route)
    B.open_tls13(batch)
    torch.cuda.synchronize()
    st, ty, cl = host_np(d_st), host_np(d_ty), host_np(d_cl).view(np.uint32)
    got = [(int(a), int(b), int(c)) for a, b, c in zip(st[:count], ty[:count], cl[:count])]
    want = [(s, t, c) for s, _, t, c in exp]
    assert got == want, (*where, "status / type / length", [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])
    assert np.array_equal(st[count:], fp.sentinel(count + PAD, 0x51)[count:]), (*where, "status tail")
    assert np.array_equal(ty[count:], fp.sentinel(count + PAD, 0x52)[count:]), (*where, "inner_type tail")
    assert np.array_equal(cl[count:], cl0[count:]), (*where, "content_len tail")
    rs = [(M + int(o), M + int(o) + max(n - 16, 0)) for o, n in zip(out_off, lens)]
    assert (d := fp.first_diff(host_np(d_out), want_img, rs)) is None, (*where, "open output", d)
    assert (d := fp.first_diff(host_np(d_in), in_img)) is None, (*where, "open input changed", d)
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
