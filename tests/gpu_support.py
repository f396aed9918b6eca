"""What the GPU tests share: device plumbing, the kernel-form switches and the
host-side description of a batch with its checkers.

Imports without torch and without a GPU (torch is imported inside the functions
that upload or download), so tests/test_gpu_support_model.py can see the
checkers fail on the CPU.  The whole-buffer comparison of
tests/test_gpu_footprint.py (footprint.first_diff) is stricter than the
per-record checkers here and stays where it is.
"""
from __future__ import annotations

import contextlib
import struct

import numpy as np
import pytest

SEED = 0x53555255
KEY = bytes(range(32))


# ---------------------------------------------------------------------------
# device plumbing
# ---------------------------------------------------------------------------
def dev_bytes(b: bytes):
    """b on the device; empty input gives a 1-byte tensor (a valid pointer)."""
    import torch

    if not b:
        return torch.zeros(1, dtype=torch.uint8, device="cuda")
    return torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")


def dev_u8(a: np.ndarray):
    import torch

    t = torch.from_numpy(np.array(a, dtype=np.uint8)).to("cuda")
    assert t.data_ptr() % 16 == 0  # the route predicates take buffer offsets for addresses
    return t


def dev_u32(vals):
    import torch

    return torch.from_numpy(np.array(vals, dtype=np.uint32).view(np.int32)).to("cuda")


def dev_u64(vals):
    import torch

    return torch.from_numpy(np.array(vals, dtype=np.uint64).view(np.int64)).to("cuda")


def host_bytes(t) -> bytes:
    return t.cpu().numpy().tobytes()


def host_np(t) -> np.ndarray:
    return t.cpu().numpy()


def filled(size: int, byte: int):
    import torch

    return torch.full((size,), byte, dtype=torch.uint8, device="cuda")


def uninit(size: int):
    """torch.empty: for an output whose every byte a record writes."""
    import torch

    return torch.empty(size, dtype=torch.uint8, device="cuda")


# ---------------------------------------------------------------------------
# kernel-form switches
# ---------------------------------------------------------------------------
SWITCHES = {"lockstep": "sg_set_lockstep", "packed": "sg_set_packed", "groups": "sg_set_msg_groups",
            "tls13_buckets": "sg_set_tls13_buckets"}


@contextlib.contextmanager
def kernel_forms(lib, **values):
    """Set the named switches (lockstep=, packed=, groups=, tls13_buckets=), check that each reads
    back, and put the previous values back on the way out."""
    prev = []
    try:
        for name, v in values.items():
            fn = getattr(lib, SWITCHES[name])
            prev.append((fn, fn(v)))
            assert fn(-1) == v, (name, v)
        yield
    finally:
        for fn, p in reversed(prev):
            fn(p)


def _switch_fixture(name):
    @pytest.fixture(name=name)
    def switch(gpu):
        """A setter for the switch; whatever a test sets is undone after it."""
        with contextlib.ExitStack() as stack:
            yield lambda v: stack.enter_context(kernel_forms(gpu, **{name: v}))

    return switch


lockstep, packed, groups = (_switch_fixture(name) for name in ("lockstep", "packed", "groups"))  # (no test asks for a fourth)


# ---------------------------------------------------------------------------
# the batch case
# ---------------------------------------------------------------------------
def slots(lens, align: int, skew=(0, 0), tail: int = 16):
    """Records one behind the other, each length (and length + tail, what it seals
    to) rounded up to `align` plus skew bytes: in_off, out_off, pt_bytes, ct_bytes."""
    lens = np.asarray(lens).astype(np.uint64)
    step_i = (lens + align - 1) // align * align + skew[0]
    step_o = (lens + tail + align - 1) // align * align + skew[1]
    in_off = np.zeros(len(lens), dtype=np.uint64)
    out_off = np.zeros(len(lens), dtype=np.uint64)
    in_off[1:] = np.cumsum(step_i[:-1])
    out_off[1:] = np.cumsum(step_o[:-1])
    return in_off, out_off, int(in_off[-1] + step_i[-1]), int(out_off[-1] + step_o[-1])


class BatchCase:
    """A batch on the host: lengths, where the records lie, the plaintext, the keys
    and the mode -- TLS (seq0 or seqs, content_type, version) or explicit (nonces_h,
    ads_h, adlen; AD stride max(adlen, 1)).

    Listed (in_off / out_off) or uniform (strides=(in_stride, out_stride)): that
    choice is the product's route, so seal_args / open_args pass arrays for the
    one and uniform_len with strides for the other and never look at the lengths.
    clamp_keys: the reference takes key min(kidx, num_keys - 1), as the kernels do.
    tail: the bytes a seal adds to a record (the tag; a TLS 1.3 record's type byte too).
    """

    def __init__(self, lens, pt_h, keys_h=KEY, *, in_off=None, out_off=None, strides=None, kidx=None,
                 clamp_keys=False, seq0=0, seqs=None, content_type=None, version=None, nonces_h=None, ads_h=None,
                 adlen=None, tail=16):
        self.lens, self.tail = np.asarray(lens).astype(np.uint32), tail
        self.count = len(self.lens)
        self.strides = strides
        if strides is not None:
            assert in_off is None and out_off is None and len(set(self.lens.tolist())) == 1
            in_off = np.arange(self.count, dtype=np.uint64) * strides[0]
            out_off = np.arange(self.count, dtype=np.uint64) * strides[1]
        self.in_off, self.out_off = in_off, out_off
        self.pt_h, self.keys_h, self.kidx, self.clamp_keys = pt_h, keys_h, kidx, clamp_keys
        self.num_keys = len(keys_h) // 32
        self.seq0, self.seqs, self.content_type, self.version = seq0, seqs, content_type, version
        self.tls = adlen is None
        self.nonces_h, self.ads_h, self.adlen = nonces_h, ads_h, adlen
        self.ad_stride = None if self.tls else max(adlen, 1)
        self._common = None

    # ---- the reference's view of record i
    def n(self, i) -> int:
        return int(self.lens[i])

    def pt(self, i) -> bytes:
        o = int(self.in_off[i])
        return bytes(self.pt_h[o:o + self.n(i)])

    def out_range(self, i):
        q = int(self.out_off[i])
        return q, q + self.n(i) + self.tail

    def key(self, i) -> bytes:
        k = 0 if self.kidx is None else int(self.kidx[i])
        if self.clamp_keys:
            k = min(k, self.num_keys - 1)
        return self.keys_h[32 * k:32 * k + 32]

    def seq(self, i) -> int:
        return int(self.seqs[i]) if self.seqs is not None else self.seq0 + i

    def nonce_ad(self, oracle, i):
        if self.tls:
            header = () if self.content_type is None else (self.content_type, *self.version)
            return struct.pack(">Q", self.seq(i)), oracle.tls_ad(self.seq(i), self.n(i), *header)
        a = i * self.ad_stride
        return bytes(self.nonces_h[8 * i:8 * i + 8]), bytes(self.ads_h[a:a + self.adlen])

    def expected(self, oracle, i) -> bytes:
        """oracle.seal of record i: ciphertext || tag."""
        nonce, ad = self.nonce_ad(oracle, i)
        return oracle.seal(self.key(i), nonce, self.pt(i), ad)

    def sealed_image(self, oracle, size: int) -> bytearray:
        """What a seal into `size` zero bytes leaves behind."""
        img = bytearray(size)
        for i in range(self.count):
            lo, hi = self.out_range(i)
            img[lo:hi] = self.expected(oracle, i)
        return img

    # ---- the Batch keywords
    def common(self, ads_h=None) -> dict:
        """count, keys, key_index and the mode; uploaded once and shared by seal and
        open (ads_h: another AD image for this call, as after tampering)."""
        if self._common is None:
            c = dict(count=self.count, keys=dev_bytes(self.keys_h).view(self.num_keys, 32))
            if self.kidx is not None:
                c["key_index"] = dev_u32(self.kidx)
            if not self.tls:
                c.update(tls=False, nonces=dev_bytes(self.nonces_h), ads=dev_bytes(bytes(self.ads_h)),
                         ad_len=self.adlen, ad_stride=self.ad_stride)
            elif self.seqs is not None:
                c["seq"] = dev_u64(self.seqs)
            else:
                c["seq0"] = self.seq0
            if self.content_type is not None:
                c.update(content_type=self.content_type, version=self.version)
            self._common = c
        if ads_h is None:
            return dict(self._common)
        return dict(self._common, ads=dev_bytes(bytes(ads_h)))

    def seal_args(self, max_len=None) -> dict:
        if self.strides is not None:
            return dict(self.common(), uniform_len=self.n(0), in_stride=self.strides[0], out_stride=self.strides[1])
        max_len = int(self.lens.max()) if max_len is None else max_len
        return dict(self.common(), lens=dev_u32(self.lens), max_len=max_len, in_off=dev_u64(self.in_off),
                    out_off=dev_u64(self.out_off))

    def open_args(self, olens=None, max_len=None, ads_h=None) -> dict:
        """The reverse direction: offsets (strides) swapped, lengths + tail unless olens says otherwise."""
        if self.strides is not None:
            return dict(self.common(ads_h), uniform_len=self.n(0) + self.tail, in_stride=self.strides[1],
                        out_stride=self.strides[0])
        olens = (self.lens + self.tail).astype(np.uint32) if olens is None else olens
        return dict(self.common(ads_h), lens=dev_u32(olens), max_len=int(olens.max()) if max_len is None else max_len,
                    in_off=dev_u64(self.out_off), out_off=dev_u64(self.in_off))


def mode_of(recs, mode, seq0=None) -> dict:
    """BatchCase's mode for records that carry their own .seq / .nonce / .ad: "tls" (their
    sequence numbers, or seq0 + i where one is given), else the explicit AD length."""
    if mode == "tls":
        return dict(seq0=seq0) if seq0 is not None else dict(seqs=np.array([r.seq for r in recs], dtype=np.uint64))
    stride = max(mode, 1)
    return dict(nonces_h=b"".join(r.nonce for r in recs), ads_h=b"".join(r.ad.ljust(stride, b"\0") for r in recs),
                adlen=mode)


# ---------------------------------------------------------------------------
# checkers: bytes or ndarrays from the host, no torch
# ---------------------------------------------------------------------------
def check_sealed(case: BatchCase, oracle, out_h, *, where=(), records=None):
    """Every record's (or every listed record's) slice of a sealed image against the reference."""
    for i in range(case.count) if records is None else records:
        lo, hi = case.out_range(i)
        assert bytes(out_h[lo:hi]) == case.expected(oracle, i), (*where, i, case.n(i))


def check_opened(case: BatchCase, back_h, st_h, exp_st, *, keep, expect_pt=None, fill=None, where=()):
    """The status bytes are exactly exp_st.  A record with status 0 is its input; with
    status 1 it is all zero, or with keep the decryption expect_pt[i] where the caller
    gives one; with status 2 or 3 it is untouched (`fill` bytes) where the caller names
    the fill, else unchecked."""
    st_h, exp_st = bytes(st_h), bytes(exp_st)
    assert len(st_h) == len(exp_st) == case.count, (*where, "status", len(st_h), len(exp_st))
    assert st_h == exp_st, (*where, "status", [(i, a, b) for i, (a, b) in enumerate(zip(st_h, exp_st)) if a != b][:5])
    for i in range(case.count):
        o, n = int(case.in_off[i]), case.n(i)
        got = bytes(back_h[o:o + n])
        if exp_st[i] == 0:
            want = case.pt(i)
        elif exp_st[i] == 1 and not keep:
            want = bytes(n)  # a record that fails its tag releases no plaintext (chacha20_poly1305.rs:89-93)
        elif exp_st[i] == 1:
            want = None if expect_pt is None or i not in expect_pt else bytes(expect_pt[i])
        else:
            want = None if fill is None else bytes([fill]) * n
        assert want is None or got == want, (*where, i, n, exp_st[i])


def xor_at(b: bytes, at: int, mask: int) -> bytes:
    """b with mask XORed into byte `at`; a position behind it (the tag) changes nothing.
    What the always-computed decryption of a tampered record is (chacha20_poly1305.rs:80-82)."""
    b = bytearray(b)
    if at < len(b):
        b[at] ^= mask
    return bytes(b)


def tamper(case: BatchCase, sealed: bytearray, flips=None, truncate=None):
    """XOR mask into byte `at` of record i for flips = {i: (at, mask)} and cut record i
    to truncate[i] < 16 bytes; returns the statuses an open must give and its lengths."""
    exp_st = bytearray(case.count)
    olens = (case.lens + 16).astype(np.uint32)
    for i, (at, mask) in (flips or {}).items():
        sealed[int(case.out_off[i]) + at] ^= mask
        exp_st[i] = 1
    for i, n in (truncate or {}).items():
        assert n < 16
        olens[i] = n
        exp_st[i] = 2
    return exp_st, olens


# ---------------------------------------------------------------------------
# one call each way; what the default would not produce is the caller's to pass
# ---------------------------------------------------------------------------
def seal(case: BatchCase, out, *, inp=None, max_len=None, **extra) -> bytearray:
    """sg_seal_batch of the case's plaintext (uploaded here unless `inp` is on the device
    already) into `out`; the sealed image on the host."""
    import torch

    from suruga_amd import batch as B

    B.seal(B.Batch(inp=dev_bytes(case.pt_h) if inp is None else inp, out=out, **case.seal_args(max_len), **extra))
    torch.cuda.synchronize()
    return bytearray(host_bytes(out))


def open_(case: BatchCase, inp, out, *, olens=None, max_len=None, ads_h=None, **extra):
    """sg_open_batch of the device buffer `inp` into `out`, the status bytes starting as
    0xFF; the output and the statuses on the host."""
    import torch

    from suruga_amd import batch as B

    st = filled(case.count, 0xFF)
    B.open_(B.Batch(inp=inp, out=out, status=st, **case.open_args(olens, max_len, ads_h), **extra))
    torch.cuda.synchronize()
    return host_bytes(out), host_bytes(st)


# ---------------------------------------------------------------------------
# the uniform TLS batch on the device's own fill rule
# ---------------------------------------------------------------------------
def tls_batch(count, n, *, seq0=0, key=KEY, j0=0):
    """Device plaintext (fill rule), sealed + opened through the batch ABI."""
    import torch

    from suruga_amd import batch as B

    keys = dev_bytes(key).view(1, 32)
    # torch.empty throughout: every byte of ct and back belongs to a record
    pt = torch.empty(count * n if n else 1, dtype=torch.uint8, device="cuda")
    if n:
        B.fill_records(pt, n, n, count, SEED, j0)
    ct = torch.empty(count * (n + 16), dtype=torch.uint8, device="cuda")
    B.seal(B.Batch(count=count, keys=keys, inp=pt, out=ct, uniform_len=n, in_stride=n, out_stride=n + 16, seq0=seq0))
    back = torch.empty(count * n if n else 1, dtype=torch.uint8, device="cuda")
    st = filled(count, 0xFF)
    B.open_(B.Batch(count=count, keys=keys, inp=ct, out=back, uniform_len=n + 16, in_stride=n + 16, out_stride=n,
                    seq0=seq0, status=st))
    torch.cuda.synchronize()
    return pt, ct, back, st
