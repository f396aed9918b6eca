"""What the TLS 1.3 bucket tests share -- TEST INFRASTRUCTURE ONLY.

sg_set_tls13_buckets as a context manager, and the routes a mixed TLS 1.3 batch must
take under it: wpr_bucket_of and pack_ok (sg_internal.h) restated on the inner lengths,
in sg_classify_kernel's order -- bucket first, then packed, else a size class.  The
layouts are tests/tls13_pad_support.py's (seal) and tests/tls13_batch_support.py's
(open); every buffer of those harnesses starts 16-byte aligned, so a record's offset
stands for its address.

Imports without torch and without a GPU."""
from __future__ import annotations

import contextlib

import tls13_pad_support as Q
from gpu_support import slots

N = 1 << 14
BUCKET_NS = (4160, 8192, 8256, 12288, 12352, 16320, 16384)
# where a content may end in its last 64-byte block: bytes 0, 1 and 15 of 16-byte units, and the block's last two
ENDS = (0, 1, 15, 16, 17, 31, 47, 62, 63)


@contextlib.contextmanager
def tls13_buckets(lib, value: int):
    """Set sg_set_tls13_buckets, check that it reads back, put the previous value back."""
    prev = lib.sg_set_tls13_buckets(value)
    try:
        assert lib.sg_set_tls13_buckets(-1) == value
        yield
    finally:
        lib.sg_set_tls13_buckets(prev)


def bucket_of(n: int, in_addr: int, out_addr: int) -> int:
    """wpr_bucket_of: J = ceil(n / 4096) = 2..4, or 0."""
    if n <= 4096 or n > N or n % 64 or (in_addr | out_addr) % 16:
        return 0
    return (n + 4095) >> 12


def pack_ok(n: int, in_addr: int, out_addr: int) -> bool:
    return 64 <= n <= 4096 and n % 64 == 0 and (in_addr | out_addr) % 16 == 0


def routes_of(inners, in_off, out_off, *, buckets: bool, packed: bool = True) -> dict:
    """What sg_last_batch_routes must say of records of these inner lengths at these offsets."""
    r = {"known": True, "classes": 0, "bucket": [0, 0, 0], "packed": 0, "skipped": 0}
    for n, i, o in zip(inners, in_off, out_off):
        J = bucket_of(n, int(i), int(o)) if buckets else 0
        if J:
            r["bucket"][J - 2] += 1
        elif packed and pack_ok(n, int(i), int(o)):
            r["packed"] += 1
        else:
            r["classes"] += 1
    return r


def seal_routes(lens, pad_to, skew=(0, 0), **kw) -> dict:
    """... of a tls13_pad_support.seal_padded of contents of these lengths."""
    inners = [Q.inner_len(n, pad_to) for n in lens]
    in_off, out_off, _, _ = Q.layout(lens, inners, skew)
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
