"""What the padded TLS 1.3 seal's GPU tests share -- TEST INFRASTRUCTURE ONLY.

tests/tls13_batch_support.py's whole-buffer seal for sg_seal_batch_tls13_ex: a record
of len content bytes seals to inner + 16 bytes, inner = inner_len(len, pad_to), so the
output slots are laid out by the inner lengths; every buffer starts as
footprint.sentinel with a margin in front and behind and is compared whole, so exactly
inner + 16 bytes per record may change and the input none.  The reference is
tests/tls13_ref.py's seal with pad = inner - len - 1.  Opening goes through
tls13_batch_support.open_whole as it is.

The second half is what the TLS 1.3 bucket tests (sg_set_tls13_buckets) add: the routes a
mixed batch must take, tests/footprint.py's route model on the inner lengths in the shape
of sg_last_batch_routes.  Every buffer of these harnesses starts 16-byte aligned, so a
record's offset stands for its address.

Imports without torch and without a GPU."""
from __future__ import annotations

import numpy as np

import footprint as fp
import tls13_batch_support as X
import tls13_ref as T
from gpu_support import slots

M = fp.MARGIN
N = 1 << 14


def inner_len(n: int, pad_to: int) -> int:
    """RFC 8446 section 5.4 as sg_tls13_inner_len states it, in Python."""
    return n + 1 if pad_to <= 1 else min(-(-(n + 1) // pad_to) * pad_to, N + 1)


def expected_padded(contents, kidx, seqs, pad_to, types, ivs=X.IVS3, keys=X.KEYS3):
    return [T.seal(*X.key_iv(int(k), ivs, keys), int(q), c, int(t), inner_len(len(c), pad_to) - len(c) - 1)
            for c, k, q, t in zip(contents, kidx, seqs, types)]


def layout(lens, inners, skew=(0, 0)):
    """Back-to-back slots of 16 bytes plus skew: content slots in, fragment slots out."""
    step_i = [fp.round_up(n, 16) + skew[0] for n in lens]
    step_o = [fp.round_up(n + 16, 16) + skew[1] for n in inners]
    in_off = np.concatenate([[0], np.cumsum(step_i[:-1])]).astype(np.uint64)
    out_off = np.concatenate([[0], np.cumsum(step_o[:-1])]).astype(np.uint64)
    return in_off, out_off, int(sum(step_i)), int(sum(step_o))


def seal_padded(contents, kidx, seqs, *, pad_to, types=None, ctype=23, skew=(0, 0), want=None, plain=False, where=()):
    """sg_seal_batch_tls13_ex (plain: sg_seal_batch_tls13, for pad_to <= 1 and one type) of
    a listed batch into a sentinel buffer.  types: a type per record, passed as the device
    array inner_types with b->content_type = `ctype` -- else every record takes ctype.
    Returns (fragments as written, last_routes() after the call, packed-eligible count)."""
    from gpu_support import dev_u8
    from suruga_amd import batch as B

    count = len(contents)
    lens = [len(c) for c in contents]
    inners = [inner_len(n, pad_to) for n in lens]
    in_off, out_off, in_size, out_size = layout(lens, inners, skew)
    each = [ctype] * count if types is None else list(types)
    want = expected_padded(contents, kidx, seqs, pad_to, each) if want is None else want
    assert [len(w) for w in want] == [n + 16 for n in inners]
    case = X.Tls13Case(lens, None, X.KEYS3, in_off=in_off, out_off=out_off, kidx=np.asarray(kidx, dtype=np.uint32),
                       seqs=np.asarray(seqs, dtype=np.uint64), ivs_h=X.IVS3, content_type=ctype, version=(3, 3), tail=17)
    in_img = np.concatenate([fp.sentinel(M, 0x31), fp.image(max(in_size, 1), 0x77, zip(in_off, contents)),
                             fp.sentinel(M, 0x32)])
    size = M + fp.round_up(out_size, 16) + M
    rs = [(M + int(o), M + int(o) + n + 16) for o, n in zip(out_off, inners)]
    got = {}

    def call(d):
        batch = B.Batch(inp=d["inp"][M:], out=d["out"][M:], **case.seal_args(max(max(lens), 1)))
        if plain:
            assert pad_to <= 1 and types is None
            B.seal_tls13(batch)
        else:
            it = None if types is None else dev_u8(np.array(each, dtype=np.uint8))
            if pad_to or it is not None:
                B.seal_tls13(batch, pad_to=pad_to, inner_types=it)
            else:
                _seal_ex(batch)
            got["types"] = it  # (alive until the run is downloaded)
        got["routes"] = B.last_routes()
        got["eligible"] = sum(fp.pack_ok(n, d["inp"][M:].data_ptr() + int(i), d["out"][M:].data_ptr() + int(o))
                              for n, i, o in zip(inners, in_off, out_off))

    o = fp.run_whole(call, in_img, fp.sentinel(size, 0x5A), fp.image(size, 0x5A, [(lo, w) for (lo, _), w in zip(rs, want)]), rs)
    o.check(where=(*where, "seal", pad_to))
    return [o.out[lo:hi].tobytes() for lo, hi in rs], got["routes"], got["eligible"]


def _seal_ex(batch):
    """sg_seal_batch_tls13_ex with {NULL, 0, 0}: the wrapper's no-argument form calls the plain entry point."""
    import ctypes as C

    from suruga_amd import _native as Nt

    cb, xb, o = batch.to_c(), batch.to_c_tls13(), Nt.SgTls13SealOpts()
    Nt.check(Nt.load().sg_seal_batch_tls13_ex(C.byref(cb), C.byref(xb), C.byref(o)))


def open_routes(frags, kidx, seqs, **kw):
    """tls13_batch_support.open_whole, then where its records went."""
    from suruga_amd import batch as B

    got = X.open_whole(frags, kidx, seqs, **kw)
    return got, B.last_routes()


# ---------------------------------------------------------------------------
# the routes of a mixed batch, buckets included
# ---------------------------------------------------------------------------
BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)
# where a content may end in its last 64-byte block: bytes 0, 1 and 15 of 16-byte units, and the block's last two
ENDS = (0, 1, 15, 16, 17, 31, 47, 62, 63)


def routes_of(inners, in_off, out_off, *, buckets: bool, packed: bool = True) -> dict:
    """What sg_last_batch_routes must say of records of these inner lengths at these offsets."""
    c = fp.route_counts(inners, in_off, out_off, buckets, packed)
    return {"known": True, "classes": sum(v for k, v in c.items() if k[0] == "class"),
            "bucket": [c.get(("bucket", J), 0) for J in (2, 3, 4)], "packed": c.get(("packed",), 0), "skipped": 0}


def seal_routes(lens, pad_to, skew=(0, 0), **kw) -> dict:
    """... of a seal_padded of contents of these lengths."""
    inners = [inner_len(n, pad_to) for n in lens]
    in_off, out_off, _, _ = layout(lens, inners, skew)
    return routes_of(inners, in_off, out_off, **kw)


def open_routes_of(frags, skew=(0, 0), **kw) -> dict:
    """... of a tls13_batch_support.open_whole of these fragments (its layout is a seal's, run backwards)."""
    inners = [max(len(f) - 16, 0) for f in frags]
    out_off, in_off, _, _ = slots(inners, 16, skew, 16)
    return routes_of(inners, in_off, out_off, **kw)


def bucket_edge_lens():
    """19 content lengths per inner length of BUCKET_NS under pad_to = 64, interleaved over the
    inner lengths: two full groups of eight and a partial one per bucket, the content ending at
    every place of ENDS."""
    return [n - 64 + ENDS[(i + j) % len(ENDS)] for i in range(19) for j, n in enumerate(BUCKET_NS)]
