"""Whole-buffer expectations for the footprint tests (tests/test_footprint_model.py
on the CPU, tests/test_gpu_footprint.py, tests/test_gpu_checkers.py and the
record-layer cases on the GPU) -- TEST INFRASTRUCTURE ONLY.

A kernel's contract is not only what it writes inside a record but that it
writes nothing else.  The tests here start every output buffer as sentinel(),
lay the records out with layout() (margins in front and behind, a cycle of gaps
between the records) and compare the *whole* buffer afterwards with image():
the sentinel with the expected bytes of every record laid over it.  run_whole()
is that run for every record and message form, Outcome.check() its one check.

The sentinel is position dependent, so that a stray store shows whatever it
stores: zeros (the scrub kernels), a fill value, keystream, or the sentinel
itself moved by a few bytes (a copy kernel that is off by one).

The route predicates restate, in Python, which kernel a record of a batch goes
to (wpr_eligible / launch_batch in sg_capi.cpp, wpr_bucket_of / pack_ok /
size_class in sg_internal.h, the comments of sg_set_lockstep / sg_set_packed in
include/suruga_gpu.h).  Every GPU case asserts with them that its records are
eligible for the route it means to exercise.  They are stated here once: the TLS
1.3 tests apply them to inner lengths (tls13_pad_support.routes_of).
"""
from __future__ import annotations

import struct
from dataclasses import dataclass, field

import numpy as np

from mac_forge import size_class  # noqa: F401  (one definition; fp.size_class stays the model's name for it)

MARGIN = 256
GAPS = (0, 1, 2, 3, 5, 8, 15, 16, 17, 63)
GAPS_ALIGNED = (0, 16, 48)
MAX_SALT_TRIES = 8

WPR_N = 16384
MAC_LEN = 16
KEY = bytes(range(9, 41))


def sentinel(size: int, salt: int = 0) -> np.ndarray:
    """Byte i = (i * 0x9D + (i >> 8) * 0x3B + salt) & 0xFF.  Neighbours differ by
    0x9D, bytes k apart by k * 0x9D (non-zero mod 256 for 0 < k < 256): no runs,
    no period of 4, 16 or 64, and no shift by 1..16 bytes maps it onto itself."""
    i = np.arange(size, dtype=np.uint64)
    return ((i * np.uint64(0x9D) + (i >> np.uint64(8)) * np.uint64(0x3B) + np.uint64(salt & 0xFF))
            & np.uint64(0xFF)).astype(np.uint8)


def round_up(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def layout(in_lens, out_lens, lead: int = MARGIN, trail: int = MARGIN, align: int = 1, gaps=None, odd=()):
    """Offsets of back-to-back records with margins and gaps.

    Record i occupies in_lens[i] bytes of the input buffer and out_lens[i]
    (its nominal output range) of the output buffer.  The gap after record i is
    gaps[i % len(gaps)] (default: GAPS, or GAPS_ALIGNED with align == 16, where
    every offset is also rounded up to 16).  Records whose index is in `odd`
    get an odd offset in both buffers (one byte more gap where needed), which
    keeps them off the 16-byte aligned routes.
    Returns (in_off, out_off, in_size, out_size), offsets as uint64 arrays."""
    assert lead >= MARGIN and trail >= MARGIN and len(in_lens) == len(out_lens)
    if gaps is None:
        gaps = GAPS_ALIGNED if align == 16 else GAPS
    res = []
    for lens in (in_lens, out_lens):
        off, pos = [], lead
        for i, n in enumerate(lens):
            pos = round_up(pos, align)
            if i in odd and pos % 2 == 0:
                pos += 1
            off.append(pos)
            pos += int(n) + gaps[i % len(gaps)]
        res.append((np.array(off, dtype=np.uint64), round_up(pos, align) + trail))
    return res[0][0], res[1][0], res[0][1], res[1][1]


def gaps_of(off, lens):
    """The gap behind every record but the last."""
    return [int(off[i + 1]) - int(off[i]) - int(lens[i]) for i in range(len(lens) - 1)]


def ranges(off, lens):
    return [(int(o), int(o) + int(n)) for o, n in zip(off, lens)]


def disjoint(rs, size: int, lead: int = MARGIN, trail: int = MARGIN) -> bool:
    """Ranges in ascending order, none overlapping, all inside [lead, size - trail]."""
    pos = lead
    for lo, hi in rs:
        if lo < pos or hi < lo:
            return False
        pos = hi
    return pos <= size - trail


def image(size: int, salt: int, parts) -> np.ndarray:
    """sentinel(size, salt) with every (offset, bytes) of parts laid over it."""
    buf = sentinel(size, salt)
    for off, b in parts:
        off = int(off)
        assert 0 <= off and off + len(b) <= size
        buf[off:off + len(b)] = np.frombuffer(bytes(b), dtype=np.uint8)
    return buf


def edges_differ(size: int, salt: int, parts) -> bool:
    """Every non-empty part differs from the bare sentinel in its first and its
    last byte: a part that equalled the sentinel there would hide a one-byte
    underwrite."""
    s = sentinel(size, salt)
    for off, b in parts:
        if len(b) and (b[0] == s[int(off)] or b[-1] == s[int(off) + len(b) - 1]):
            return False
    return True


def pick_salt(size: int, parts, first: int = 0):
    """(salt, tries): the first salt from `first` on under which edges_differ
    holds; at most MAX_SALT_TRIES are tried (the callers assert tries <= that)."""
    for t in range(MAX_SALT_TRIES):
        salt = (first + 37 * t) & 0xFF
        if edges_differ(size, salt, parts):
            return salt, t + 1
    raise AssertionError(f"no salt in {MAX_SALT_TRIES} tries keeps every record edge off the sentinel")


def first_diff(got: np.ndarray, want: np.ndarray, rs=()):
    """None when equal, else a description of the first differing byte: its
    position, and the record range it lies in or the ranges it lies between."""
    assert got.shape == want.shape
    d = np.flatnonzero(got != want)
    if d.size == 0:
        return None
    p = int(d[0])
    where = "outside every record"
    for i, (lo, hi) in enumerate(rs):
        if lo <= p < hi:
            where = f"record {i} byte {p - lo} of {hi - lo}"
            break
        if p < lo:
            where = f"{lo - p} bytes before record {i}" + (f", {p - rs[i - 1][1]} behind record {i - 1}" if i else "")
            break
    else:
        if rs:
            where = f"{p - rs[-1][1]} bytes behind the last record"
    return f"byte {p}: got {int(got[p]):#04x} want {int(want[p]):#04x} ({where}; {d.size} bytes differ)"


# ---------------------------------------------------------------------------
# one whole-buffer run: the images around a call and their one check
# ---------------------------------------------------------------------------
ARRAY_PAD = 64  # sentinel entries behind the `count` entries of a per-record output array


def array_start(count: int, salt: int, dtype=np.uint8) -> np.ndarray:
    """A per-record output array (status, inner_type, content_len) before the call:
    count entries and ARRAY_PAD behind them, all sentinel."""
    return sentinel(np.dtype(dtype).itemsize * (count + ARRAY_PAD), salt).view(dtype)


@dataclass
class Array:
    got: np.ndarray    # the whole array after the call
    start: np.ndarray  # ... and as it was uploaded


@dataclass
class Outcome:
    """What a call left behind, whole, beside what it had to leave."""

    out: np.ndarray       # the whole output buffer
    want_out: np.ndarray
    out_ranges: list      # the records' nominal output ranges (for the message of a difference)
    inp: np.ndarray       # the whole input buffer (records in place write here)
    want_inp: np.ndarray
    in_ranges: list = ()
    arrays: dict = field(default_factory=dict)  # name -> Array, in the order check() takes their values
    ret: object = None    # what the call returned

    def check(self, *want, where=()):
        """The output is want_out and the input want_inp, byte for byte; array k holds
        want[k] in its first len(want[k]) entries and is otherwise untouched (no or a
        None want[k]: the whole array is)."""
        d = first_diff(self.out, self.want_out, self.out_ranges)
        assert d is None, (*where, "output", d)
        d = first_diff(self.inp, self.want_inp, self.in_ranges)
        assert d is None, (*where, "input", d)
        assert len(want) <= len(self.arrays)
        for k, (name, a) in enumerate(self.arrays.items()):
            w = [int(v) for v in want[k]] if k < len(want) and want[k] is not None else []
            got = a.got[:len(w)].tolist()
            assert got == w, (*where, name, [(i, g, v) for i, (g, v) in enumerate(zip(got, w)) if g != v][:8])
            assert a.got.shape == a.start.shape and np.array_equal(a.got[len(w):], a.start[len(w):]), (*where, name + " tail")


def run_whole(call, inp, out, want_out, out_ranges, *, want_inp=None, in_ranges=(), arrays=None, sync=True):
    """Upload the input image, the output buffer's start image and the named
    per-record arrays (each 16-byte aligned: gpu_support.dev_u8), call(dev) with the
    device tensors by name ("inp", "out", the arrays' names; all uint8), wait and
    download everything into an Outcome.  sync=False: the function that waits and
    returns it."""
    import torch

    from gpu_support import dev_u8, host_np

    arrays = arrays or {}
    dev = {k: dev_u8(v.view(np.uint8)) for k, v in dict(inp=inp, out=out, **arrays).items()}
    ret = call(dev)

    def finish():
        torch.cuda.synchronize()
        got = {k: host_np(t) for k, t in dev.items()}  # (dev: the buffers live until the work is done)
        return Outcome(got["out"], want_out, out_ranges, got["inp"], inp if want_inp is None else want_inp, in_ranges,
                       {k: Array(got[k].view(v.dtype), v) for k, v in arrays.items()}, ret)

    return finish() if sync else finish


# ---------------------------------------------------------------------------
# route predicates (n: plaintext bytes of the record)
# ---------------------------------------------------------------------------
def uniform_wpr(n: int, listed: bool, in_base: int, out_base: int, in_stride: int, out_stride: int,
                lockstep: bool = True) -> bool:
    """wpr_eligible: a uniform batch (no len / offset arrays) of full 16 KiB
    records in a 16-byte aligned strided layout, lock-step switch on."""
    return (lockstep and not listed and n == WPR_N
            and (in_base | out_base | in_stride | out_stride) % 16 == 0)


def mixed_routes(max_n: int, tls: bool, listed: bool, lockstep: bool = True, packed: bool = True):
    """launch_batch: (buckets on, packed on) for a batch whose longest admitted
    record has max_n plaintext bytes.  Only a TLS batch with a len array and
    records in more than the lowest size class is bucketed that way (the
    per-record arrays 4-byte aligned, which device allocations are)."""
    if not (listed and tls and size_class(max_n) != 0):
        return False, False
    if not ((lockstep and max_n > 4096) or (packed and max_n >= 64)):
        return False, False
    return lockstep and max_n > 4096, packed


def bucket_of(n: int, in_addr: int, out_addr: int) -> int:
    """wpr_bucket_of: J = ceil(n / 4096) = 2..4, or 0."""
    if n <= 4096 or n > WPR_N or n % 64 or (in_addr | out_addr) % 16:
        return 0
    return (n + 4095) >> 12


def pack_ok(n: int, in_addr: int, out_addr: int) -> bool:
    return 64 <= n <= 4096 and n % 64 == 0 and (in_addr | out_addr) % 16 == 0


def route(n: int, in_addr: int, out_addr: int, buckets: bool, packed: bool):
    """The list of one record of a mixed batch: ("bucket", J), ("packed",) or
    ("class", c) -- sg_classify_kernel's order."""
    J = bucket_of(n, in_addr, out_addr) if buckets else 0
    if J:
        return ("bucket", J)
    if packed and pack_ok(n, in_addr, out_addr):
        return ("packed",)
    return ("class", size_class(n))


def route_counts(ns, in_addrs, out_addrs, buckets: bool, packed: bool) -> dict:
    out: dict = {}
    for n, a, b in zip(ns, in_addrs, out_addrs):
        r = route(int(n), int(a), int(b), buckets, packed)
        out[r] = out.get(r, 0) + 1
    return out


# ---------------------------------------------------------------------------
# the batches of tests/test_gpu_footprint.py (lengths only; the CPU test checks
# their layouts and routes with device bases that are 16-byte aligned)
# ---------------------------------------------------------------------------
SC_LENGTHS = (100, 200, 400, 800, 1600, 3200, 6400, 12800)  # mac_forge.SC_LENGTHS
PACKED_LENGTHS = (64, 128, 1024, 4096)
BUCKET_LENGTHS = (4160, 8192, 8256, 12288, 12352, 16384)
EDGE_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65)
UNIFORM_LENGTHS = SC_LENGTHS + EDGE_LENGTHS
UNIFORM_GAPS = (0, 1, 3, 16)
UNIFORM_BASES = (0, 1)
UNIFORM_COUNT = 5
WPR_PADS = (0, 16, 48)
WPR_COUNTS = (1, 5, 9, 23)
LISTED_MODES = ("tls", 0, 7, 29)


def listed_lengths():
    """The mixed batch through the list-driven size classes: (lens, odd) -- the
    lengths the packed and bucket kernels would take sit at odd offsets."""
    plain = SC_LENGTHS + EDGE_LENGTHS + (4097, 16383, 16384)
    forced = PACKED_LENGTHS + BUCKET_LENGTHS
    lens, odd = [], set()
    for rep in range(3):
        for n in plain:
            lens.append(n)
        for n in forced:
            odd.add(len(lens))
            lens.append(n)
    # 64 and 16384 are in both lists: every copy goes odd
    odd.update(i for i, n in enumerate(lens) if n in forced)
    return lens, odd


def packed_lengths():
    """300 records of the packed kernel (two full 128-record runs and a partial
    one): every multiple of 64 up to 4096, small ones more often."""
    lens = [64 * (1 + i) for i in range(64)]
    lens += [64 * (1 + (7 * i) % 16) for i in range(236)]
    assert len(lens) == 300
    return lens


def bucket_lengths(times: int):
    return [n for _ in range(times) for n in BUCKET_LENGTHS]


def packed_and_bucket_lengths():
    """The packed batch with every bucket length mixed in four times."""
    lens = packed_lengths()
    for k, n in enumerate(bucket_lengths(4)):
        lens.insert(11 * k + 5, n)
    return lens


# ---------------------------------------------------------------------------
# a listed batch with its two records that must stay untouched
# ---------------------------------------------------------------------------
SHORT_IN, SHORT_NOMINAL = 7, 24  # open: 7 input bytes (status 2), a nominal output range of 24


class Plan:
    """The layout of one listed batch, both directions.

    all_lens: plaintext lengths, with a short record at index i_short (sealed
    as an ordinary 7-byte record; on open its input is those 7 bytes, shorter
    than a tag) and one of max + 64 bytes, longer than max_len, at i_long.
    seal / open: (in_lens, out_lens, in_off, out_off, in_size, out_size)."""

    def __init__(self, name, lens, odd=(), align: int = 1):
        lens = [int(n) for n in lens]
        self.name = name
        self.max_n = max(lens)
        self.i_short, self.i_long = 3, len(lens) // 2
        assert self.i_long > self.i_short
        self.all_lens = list(lens)
        self.all_lens.insert(self.i_short, SHORT_IN)
        self.all_lens.insert(self.i_long, self.max_n + 64)
        moved = lambda j: j + (j >= self.i_short)
        self.odd = {moved(j) + (moved(j) >= self.i_long) for j in odd}
        self.count = len(self.all_lens)
        self.ordinary = [i for i in range(self.count) if i not in (self.i_short, self.i_long)]
        s_in, s_out = list(self.all_lens), [n + MAC_LEN for n in self.all_lens]
        self.seal = (s_in, s_out) + layout(s_in, s_out, align=align, odd=self.odd)
        o_in, o_out = [n + MAC_LEN for n in self.all_lens], list(self.all_lens)
        o_in[self.i_short], o_out[self.i_short] = SHORT_IN, SHORT_NOMINAL
        self.open = (o_in, o_out) + layout(o_in, o_out, align=align, odd=self.odd)

    def routes(self, direction, tls: bool, lockstep: bool = True, packed: bool = True, base: int = 0) -> dict:
        """Route populations of the ordinary records (base: the buffers' address mod 16)."""
        _, _, in_off, out_off, _, _ = direction
        buckets, pk = mixed_routes(self.max_n, tls, True, lockstep, packed)
        idx = self.ordinary
        return route_counts([self.all_lens[i] for i in idx], [base + int(in_off[i]) for i in idx],
                            [base + int(out_off[i]) for i in idx], buckets, pk)


def listed_plan():
    lens, odd = listed_lengths()
    return Plan("listed", lens, odd, 1)


def packed_plan():
    return Plan("packed", packed_and_bucket_lengths(), (), 16)


def bucket_plan():
    return Plan("bucket", bucket_lengths(6), (), 16)


def expect_listed_routes(counts: dict, all_classes_only: bool):
    for c in range(8):
        assert counts.get(("class", c), 0) >= 3, (c, counts)
    if all_classes_only:
        assert all(k[0] == "class" for k in counts), counts


def expect_packed_routes(counts: dict):
    assert counts.get(("packed",), 0) == 300, counts
    assert [counts.get(("bucket", J), 0) for J in (2, 3, 4)] == [8, 8, 8], counts


def expect_bucket_routes(counts: dict):
    assert [counts.get(("bucket", J), 0) for J in (2, 3, 4)] == [12, 12, 12], counts


# ---------------------------------------------------------------------------
# records (sealed by the oracle; cached per batch)
# ---------------------------------------------------------------------------
class Rec:
    """One record: plaintext, nonce, AD and what the oracle seals it to."""

    def __init__(self, oracle, rng, n: int, mode, seq: int):
        self.pt = rng.bytes(n)
        if mode == "tls":
            self.nonce, self.ad = struct.pack(">Q", seq), oracle.tls_ad(seq, n)
        else:
            self.nonce, self.ad = rng.bytes(8), rng.bytes(mode)
        self.sealed = oracle.seal(KEY, self.nonce, self.pt, self.ad)
        self.oracle = oracle

    def tampered(self, i: int) -> bytes:
        b = bytearray(self.sealed)
        b[(131 * i + 5) % len(b)] ^= 1 << (i % 8)
        return bytes(b)

    def decrypted(self, data: bytes) -> bytes:
        """The always-computed decryption of a failed open (chacha20_poly1305.rs:80-82)."""
        rc, pt = self.oracle.open(KEY, self.nonce, data, self.ad)
        assert rc == 1  # SG_E_BAD_MAC
        return pt


_cache: dict = {}


def records(oracle, lens, mode, seq0: int):
    key = (tuple(lens), mode, seq0)
    if key not in _cache:
        rng = np.random.default_rng([len(lens), seq0, 0 if mode == "tls" else 1 + mode])
        _cache[key] = [Rec(oracle, rng, n, mode, seq0 + i) for i, n in enumerate(lens)]
    return _cache[key]


def is_tampered(i: int) -> bool:
    """About one record in seven of the tampered directions."""
    return i % 7 == 3


# ---------------------------------------------------------------------------
# the expected images of a plan, shared by the CPU and the GPU test
# ---------------------------------------------------------------------------
OPEN_VARIANTS = (("open", False, False), ("open tampered", True, False), ("open tampered keep_failed", True, True))


def seal_parts(plan: Plan, recs):
    """What a seal of the plan writes: every record but the over-long one."""
    out_off = plan.seal[3]
    return [(out_off[i], recs[i].sealed) for i in range(plan.count) if i != plan.i_long]


def open_case(plan: Plan, recs, tamper: bool, keep: bool):
    """(inputs, parts, statuses) of one open of the plan."""
    out_off = plan.open[3]
    inputs, parts, st = [], [], []
    for i, r in enumerate(recs):
        if i == plan.i_short:
            inputs.append(r.pt)
            st.append(2)
        elif i == plan.i_long:
            inputs.append(r.sealed)
            st.append(3)
        elif tamper and is_tampered(i):
            inputs.append(r.tampered(i))
            parts.append((out_off[i], r.decrypted(inputs[-1]) if keep else bytes(plan.all_lens[i])))
            st.append(1)
        else:
            inputs.append(r.sealed)
            parts.append((out_off[i], r.pt))
            st.append(0)
    return inputs, parts, st


PLAN_SEQ0 = 500
# A batch of r records has 2 r edges, each of which rules out one of the 256
# salts: the packed batch (326 records) leaves about 20 salts free, and a blind
# search from an arbitrary start needs about 12 tries.  Every search over a
# plan's images starts at PLAN_SALT, from where each ends within
# MAX_SALT_TRIES; tests/test_footprint_model.py holds that for exactly the
# images the GPU test builds (plan_images).
PLAN_SALT = 0x11


def plan_images(plan: Plan, recs):
    """Every (what, out_size, parts, salt, tries) the GPU test builds from the plan."""
    out = []
    cases = [("seal", plan.seal[5], seal_parts(plan, recs))]
    cases += [(what, plan.open[5], open_case(plan, recs, tamper, keep)[1]) for what, tamper, keep in OPEN_VARIANTS]
    for what, size, parts in cases:
        salt, tries = pick_salt(size, parts, PLAN_SALT)
        out.append((what, size, parts, salt, tries))
    return out
