"""What the GPU tests of the RFC 7905 / TLS 1.3 record layer share -- TEST
INFRASTRUCTURE ONLY: contexts with a write IV, caller buffers inside sentinel
margins at a chosen misalignment (pageable or registered), the write and read
calls with whole-buffer checks, and the batch calls the written wire is held
against.  Imports without torch and without a GPU."""
from __future__ import annotations

import contextlib
import ctypes as C

import numpy as np

import footprint as fp
import record13_ref as RR

MARGIN = 256
SLOT = 18432
FORMS = ("tls13", "rfc7905")


def new_ctx(lib, key: bytes = RR.KEY, iv=RR.IV):
    from suruga_amd import _native as N

    ptr = lib.sg_ctx_new(key, 0)
    assert ptr
    if iv is not None:
        N.check(lib.sg_ctx_set_iv(ptr, iv))
    return ptr


@contextlib.contextmanager
def context(lib, key: bytes = RR.KEY, iv=RR.IV):
    ptr = new_ctx(lib, key, iv)
    try:
        yield ptr
    finally:
        lib.sg_ctx_free(ptr)


class Buf:
    """n caller bytes at `off` bytes past 64-byte alignment, inside sentinel margins."""

    def __init__(self, n: int, off: int = 0, salt: int = 0x5A, fill: bytes | None = None):
        size = MARGIN + off + n + MARGIN
        raw = np.empty(size + 64, dtype=np.uint8)
        skip = (-raw.ctypes.data) % 64
        self.arr = raw[skip:skip + size]
        self.start = fp.sentinel(size, salt)
        self.arr[:] = self.start
        self.lo, self.hi = MARGIN + off, MARGIN + off + n
        if fill is not None:
            self.arr[self.lo:self.hi] = np.frombuffer(fill, dtype=np.uint8)
            self.start = self.arr.copy()
        assert (self.arr.ctypes.data + MARGIN) % 64 == 0

    @property
    def ptr(self) -> int:
        return self.arr.ctypes.data + self.lo

    @property
    def n(self) -> int:
        return self.hi - self.lo

    def window(self) -> np.ndarray:
        return self.arr[self.lo:self.hi]

    def reset(self) -> None:
        self.arr[:] = self.start

    def check(self, written: bytes, what: str, zero_ok_from: int | None = None) -> None:
        """The whole array is its start image with `written` laid over the window's
        beginning.  zero_ok_from: window bytes from there on may also be zero."""
        want = self.start.copy()
        want[self.lo:self.lo + len(written)] = np.frombuffer(written, dtype=np.uint8)
        got = self.arr
        if zero_ok_from is not None:
            got = got.copy()
            tail = got[self.lo + zero_ok_from:self.hi]
            tail[tail == 0] = want[self.lo + zero_ok_from:self.hi][tail == 0]
        d = fp.first_diff(got, want, [(self.lo, self.lo + len(written))])
        assert d is None, f"{what}: {d}"


@contextlib.contextmanager
def registered(lib, bufs, on: bool):
    from suruga_amd import _native as N

    done = []
    try:
        if on:
            for b in bufs:
                N.check(lib.sg_host_register(b.arr.ctypes.data, b.arr.nbytes))
                done.append(b)
        yield
    finally:
        for b in done:
            N.check(lib.sg_host_unregister(b.arr.ctypes.data))


def write(lib, form: str, ctx, seq0: int, ctype: int, data: Buf, wire: Buf):
    """-> (return value, wire_len)"""
    wl = C.c_size_t(0)
    if form == "tls13":
        rc = lib.sg_write_records_tls13(ctx, seq0, ctype, data.ptr, data.n, wire.ptr, wire.n, C.byref(wl))
    else:
        rc = lib.sg_write_records_rfc7905(ctx, seq0, ctype, 3, 3, data.ptr, data.n, wire.ptr, wire.n, C.byref(wl))
    return rc, wl.value


def read(lib, form: str, ctx, seq0: int, wire: Buf, out: Buf, max_records: int = 1 << 12):
    """-> record13_ref.Read of what the call delivered (out: the first out_len bytes)."""
    from suruga_amd import _native as N

    types = np.full(max_records, 0xEE, dtype=np.uint8)
    lens = np.full(max_records, 0xEEEEEEEE, dtype=np.uint32)
    res = N.SgReadResult()
    fn = lib.sg_read_records_tls13 if form == "tls13" else lib.sg_read_records_rfc7905
    N.check(fn(ctx, seq0, wire.ptr, wire.n, out.ptr, out.n, types.ctypes.data, lens.ctypes.data, max_records,
               C.byref(res)))
    k = int(res.records)
    assert np.all(types[k:] == 0xEE) and np.all(lens[k:] == 0xEEEEEEEE), "types / frag_lens written beyond `records`"
    return RR.Read(types[:k].tolist(), lens[:k].tolist(), out.window()[:res.out_len].tobytes(), k, int(res.consumed),
                   int(res.out_len), int(res.error))


def check_read(got: RR.Read, want: RR.Read, what: str) -> None:
    assert (got.records, got.consumed, got.out_len, got.error) == (want.records, want.consumed, want.out_len,
                                                                     want.error), what
    assert got.types == want.types and got.lens == want.lens, what
    assert got.out == want.out, what


def batch_fragments(lib, form: str, seq0: int, ctype: int, pts, key: bytes = RR.KEY, iv: bytes = RR.IV):
    """The fragments sg_seal_batch_tls13 / sg_seal_batch_rfc8439 (TLS mode) give for
    the plaintexts `pts`, records at 16-byte aligned slots."""
    import torch

    from gpu_support import dev_bytes, dev_u32
    from suruga_amd import _native as N

    count = len(pts)
    inp = np.zeros(count * SLOT, dtype=np.uint8)
    for i, p in enumerate(pts):
        inp[i * SLOT:i * SLOT + len(p)] = np.frombuffer(p, dtype=np.uint8)
    d_in = torch.from_numpy(inp).to("cuda")
    d_out = torch.zeros(count * SLOT, dtype=torch.uint8, device="cuda")
    d_key, d_iv, d_len = dev_bytes(key), dev_bytes(iv + bytes(4)), dev_u32([len(p) for p in pts])
    b = N.SgBatch()
    b.count, b.flags, b.keys, b.num_keys, b.seq0 = count, N.SG_BATCH_TLS, d_key.data_ptr(), 1, seq0
    b.content_type, b.ver_major, b.ver_minor = ctype, 3, 3
    b.in_, b.in_stride, b.out, b.out_stride = d_in.data_ptr(), SLOT, d_out.data_ptr(), SLOT
    b.len, b.max_len = d_len.data_ptr(), RR.FULL
    if form == "tls13":
        x = N.SgBatchTls13()
        x.ivs = d_iv.data_ptr()
        N.check(lib.sg_seal_batch_tls13(C.byref(b), C.byref(x)))
        extra = 17
    else:
        x = N.SgBatchRfc8439()
        x.ivs = d_iv.data_ptr()
        N.check(lib.sg_seal_batch_rfc8439(C.byref(b), C.byref(x)))
        extra = 16
    torch.cuda.synchronize()
    out = d_out.cpu().numpy()
    return [out[i * SLOT:i * SLOT + len(p) + extra].tobytes() for i, p in enumerate(pts)]


def framed(form: str, ctype: int, frags) -> bytes:
    import struct

    ty = 23 if form == "tls13" else ctype
    return b"".join(struct.pack(">BBBH", ty, 3, 3, len(f)) + f for f in frags)


def ref_record(form: str, seq: int, ctype: int, pt: bytes, key: bytes = RR.KEY, iv: bytes = RR.IV) -> bytes:
    it = RR.Item(pt, ctype)
    return RR.record13(key, iv, seq, it) if form == "tls13" else RR.record7905(key, iv, seq, it)
