"""Every kernel writes only its own bytes.

The batch ABI promises that record i writes out + out_off_i, len_i + 16 bytes on
seal and len_i - 16 on open, and nothing else; that a record too short to hold
a tag writes nothing; that a record longer than max_len is left untouched.  The
message ABI makes the same promise.  Here every output buffer starts as a
position-dependent sentinel (tests/footprint.py), the records lie between
margins of 256 bytes and gaps of 0..63 bytes, and after the call the *whole*
buffer -- margins, gaps and the ranges of the records that must stay untouched
included -- equals the sentinel with oracle.seal / the plaintext / zeros / the
oracle's unauthenticated decryption laid over it.  The input buffer is byte for
byte what was uploaded, and a status array with 64 sentinel bytes behind it is
unchanged past `count`.

Four directions per case: seal, open, open with about one record in seven
tampered (scrubbed to zeros), and the same with SG_BATCH_KEEP_FAILED.  Every
listed batch carries a record shorter than a tag (status 2, with a non-empty
nominal output range) and one longer than max_len (status 3, SG_E_ARG).  Every
case asserts with the route predicates of tests/footprint.py that its records
go where the case means them to go.

Out of scope: the device group counter walk of the wave-per-record bucket
kernel, which needs thousands of records per bucket; its stores are the same
code as the ones exercised here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import footprint as fp
import mac_forge as F
from gpu_support import BatchCase, dev_u8 as to_dev, dev_u32, dev_u64, host_np as host, mode_of
from gpu_support import groups, lockstep, packed  # noqa: F401  (fixtures)
from suruga_amd._native import SG_E_ARG, SG_E_BAD_MAC, SG_E_SHORT, SG_OK

pytestmark = pytest.mark.gpu

KEY = fp.KEY
M = fp.MARGIN
STATUS_PAD = 64


def u8(b: bytes) -> np.ndarray:
    return np.frombuffer(bytes(b), dtype=np.uint8)


records, is_tampered = fp.records, fp.is_tampered


def common_args(recs, mode, seq0) -> dict:
    """count, keys, the mode and the NULL stream (every call here ends before it returns)."""
    case = BatchCase(np.zeros(len(recs)), None, KEY, **mode_of(recs, mode, seq0))
    return dict(case.common(), stream=0)


def call(gpu, batch, open_: bool) -> int:
    import torch

    cb = batch.to_c()
    rc = (gpu.sg_open_batch if open_ else gpu.sg_seal_batch)(C.byref(cb))
    torch.cuda.synchronize()
    return rc


def run_whole(gpu, what, batch_args: dict, open_, in_img, out_size, salt, parts, out_ranges, st_want=None, lead=0):
    """One batch call on whole images (footprint.run_whole): inp / out from byte `lead` of the
    uploaded buffers, an open's status array with its sentinel tail; returns the call's code
    after the whole-buffer check."""
    from suruga_amd import batch as B

    count = len(out_ranges)
    arrays = {"status": fp.array_start(count, 0x51)} if open_ else {}
    o = fp.run_whole(lambda d: call(gpu, B.Batch(inp=d["inp"][lead:], out=d["out"][lead:], status=d.get("status"), **batch_args),
                                    open_),
                     in_img, fp.sentinel(out_size, salt), fp.image(out_size, salt, parts), out_ranges, arrays=arrays)
    o.check(*([st_want] if open_ else []), where=(what,))
    return o.ret


# ---------------------------------------------------------------------------
# listed (mixed) batches
# ---------------------------------------------------------------------------
def run_listed(gpu, oracle, plan, mode, expect_routes, lockstep_on=True, packed_on=True, seq0=fp.PLAN_SEQ0):
    """plan: footprint.Plan -- the ordinary records, a short one (status 2, with a
    nominal output range) at plan.i_short and one longer than max_len at plan.i_long.
    expect_routes(counts): asserts on the route populations of the ordinary records."""
    all_lens, count, max_n, i_short, i_long = plan.all_lens, plan.count, plan.max_n, plan.i_short, plan.i_long
    recs = records(oracle, all_lens, mode, seq0)
    tls = mode == "tls"

    # ---- seal: the short record is an ordinary 7-byte one, the long one is skipped
    in_lens, out_lens, in_off, out_off, in_size, out_size = plan.seal
    assert fp.disjoint(fp.ranges(in_off, in_lens), in_size) and fp.disjoint(fp.ranges(out_off, out_lens), out_size)
    expect_routes(plan.routes(plan.seal, tls, lockstep_on, packed_on))
    parts = fp.seal_parts(plan, recs)
    salt, tries = fp.pick_salt(out_size, parts, fp.PLAN_SALT)
    assert tries <= fp.MAX_SALT_TRIES
    in_img = fp.image(in_size, 0x77, [(in_off[i], recs[i].pt) for i in range(count)])
    common = common_args(recs, mode, seq0)
    rc = run_whole(gpu, "seal", dict(lens=dev_u32(in_lens), max_len=max_n, in_off=dev_u64(in_off), out_off=dev_u64(out_off),
                                     **common), False, in_img, out_size, salt, parts, fp.ranges(out_off, out_lens))
    assert rc == SG_E_ARG, "seal: a record longer than max_len returns SG_E_ARG"

    # ---- open
    in_lens, out_lens, in_off, out_off, in_size, out_size = plan.open
    assert fp.disjoint(fp.ranges(in_off, in_lens), in_size) and fp.disjoint(fp.ranges(out_off, out_lens), out_size)
    expect_routes(plan.routes(plan.open, tls, lockstep_on, packed_on))
    d_lens, d_io, d_oo = dev_u32(in_lens), dev_u64(in_off), dev_u64(out_off)
    for what, tamper, keep in fp.OPEN_VARIANTS:
        inputs, parts, st_want = fp.open_case(plan, recs, tamper, keep)
        salt, tries = fp.pick_salt(out_size, parts, fp.PLAN_SALT)
        assert tries <= fp.MAX_SALT_TRIES
        in_img = fp.image(in_size, 0x78, [(in_off[i], inputs[i]) for i in range(count)])
        rc = run_whole(gpu, what, dict(lens=d_lens, max_len=max_n + 16, in_off=d_io, out_off=d_oo, keep_failed=keep, **common),
                       True, in_img, out_size, salt, parts, fp.ranges(out_off, out_lens), st_want)
        assert rc == SG_E_ARG, f"{what}: a record longer than max_len returns SG_E_ARG"


@pytest.mark.parametrize("switches", ["default", "off"])
@pytest.mark.parametrize("mode", fp.LISTED_MODES)
def test_listed_size_classes(gpu, oracle, lockstep, packed, mode, switches):
    """Every size class from its list, byte-granular offsets; the lengths the packed
    and bucket kernels would take sit at odd offsets (and, with both switches off,
    anywhere) and fall back to the classes."""
    on = switches == "default"
    lockstep(1 if on else 0)
    packed(1 if on else 0)
    run_listed(gpu, oracle, fp.listed_plan(), mode,
               lambda c: fp.expect_listed_routes(c, not on or mode != "tls"), on, on)


def test_packed_kernel_and_buckets(gpu, oracle, lockstep, packed):
    """300 records of the packed kernel (two full 128-record runs and a partial
    one, every multiple of 64 up to 4096) with each bucket length four times
    among them, 16-byte aligned with gaps of 0, 16 and 48."""
    lockstep(1)
    packed(1)
    run_listed(gpu, oracle, fp.packed_plan(), "tls", fp.expect_packed_routes)


def test_wave_per_record_buckets(gpu, oracle, lockstep, packed):
    """A batch of the bucket lengths alone (first and last length of J = 2, 3, 4), six times each."""
    lockstep(1)
    packed(1)
    run_listed(gpu, oracle, fp.bucket_plan(), "tls", fp.expect_bucket_routes)


# ---------------------------------------------------------------------------
# uniform batches
# ---------------------------------------------------------------------------
def run_uniform(gpu, oracle, n, count, mode, gaps, bases, want_wpr, seq0=77):
    """len = NULL; seal strides n + g -> n + 16 + g, open the reverse, buffers at base b."""
    recs = records(oracle, [n] * max(count, max(fp.WPR_COUNTS) if n == fp.WPR_N else 0), mode, seq0)[:count]
    common = common_args(recs, mode, seq0)

    def one(what, open_, inputs, outputs, in_len, out_len, g, b, st_want, keep=False):
        si, so = in_len + g, out_len + g
        assert fp.uniform_wpr(n, False, b, b, si, so) == want_wpr, (what, n, g, b)
        in_size, out_size = 2 * M + b + count * si, 2 * M + b + count * so
        parts = [(M + b + i * so, o) for i, o in enumerate(outputs) if o is not None]
        salt, tries = fp.pick_salt(out_size, parts, 0x35)
        assert tries <= fp.MAX_SALT_TRIES
        in_img = fp.image(in_size, 0x79, [(M + b + i * si, x) for i, x in enumerate(inputs)])
        what = f"{what} n={n} count={count} g={g} base={b}"
        rc = run_whole(gpu, what, dict(uniform_len=in_len, in_stride=si, out_stride=so, keep_failed=keep, **common), open_,
                       in_img, out_size, salt, parts, [(M + b + i * so, M + b + i * so + out_len) for i in range(count)],
                       st_want, lead=M + b)
        assert rc == SG_OK, what

    for g in gaps:
        for b in bases:
            one("seal", False, [r.pt for r in recs], [r.sealed for r in recs], n, n + 16, g, b, None)
            for what, tamper, keep in fp.OPEN_VARIANTS:
                inputs, outputs, st = [], [], []
                for i, r in enumerate(recs):
                    bad = tamper and (is_tampered(i) or count == 1)
                    inputs.append(r.tampered(i) if bad else r.sealed)
                    outputs.append((r.decrypted(inputs[-1]) if keep else bytes(n)) if bad else r.pt)
                    st.append(1 if bad else 0)
                one(what, True, inputs, outputs, n + 16, n, g, b, st, keep)
            if n < 16:  # every record shorter than a tag: status 2, nothing written
                one("open short", True, [r.pt for r in recs], [None] * count, n, fp.SHORT_NOMINAL, g, b, [2] * count)


@pytest.mark.parametrize("n", fp.UNIFORM_LENGTHS)
def test_uniform_size_classes(gpu, oracle, lockstep, n):
    """Direct launch of one size class: odd strides and an odd base."""
    lockstep(1)
    run_uniform(gpu, oracle, n, fp.UNIFORM_COUNT, "tls", fp.UNIFORM_GAPS, fp.UNIFORM_BASES, False)


@pytest.mark.parametrize("mode", ["tls", 0, 255])
def test_uniform_wave_per_record(gpu, oracle, lockstep, mode):
    """16 KiB records right-aligned in their frames; strides padded by 0, 16 and
    48 bytes; 1 record, part of a workgroup, one more than a workgroup, 23."""
    lockstep(1)
    for count in fp.WPR_COUNTS:
        run_uniform(gpu, oracle, fp.WPR_N, count, mode, fp.WPR_PADS, (0,), True)


# ---------------------------------------------------------------------------
# long message, device form
# ---------------------------------------------------------------------------
MSG_AD = bytes(range(100, 113))
MSG_OFFSETS = (0, 1, 3, 15)


def msg_lengths():
    T = F.tile_bytes()
    return (T - 1, T, T + 1, 2 * T + 33, 0, 1, 15, 16, 17)


class MsgRec:
    def __init__(self, oracle, n):
        rng = np.random.default_rng([n, 99])
        self.n, self.pt, self.nonce, self.oracle = n, rng.bytes(n), rng.bytes(8), oracle
        self.sealed = oracle.seal(KEY, self.nonce, self.pt, MSG_AD)
        b = bytearray(self.sealed)
        b[(n * 7) % len(b)] ^= 0x20
        self.bad = bytes(b)
        rc, self.bad_pt = oracle.open(KEY, self.nonce, self.bad, MSG_AD)
        assert rc == SG_E_BAD_MAC


_msg_cache: dict = {}


def msg_rec(oracle, n):
    if n not in _msg_cache:
        _msg_cache[n] = MsgRec(oracle, n)
    return _msg_cache[n]


def msg_cases(r):
    """(name, input, expected output, status, keep_failed); status None: seal."""
    return (("seal", r.pt, r.sealed, None, False), ("open", r.sealed, r.pt, 0, False),
            ("open tampered", r.bad, bytes(r.n), 1, False), ("open tampered keep_failed", r.bad, r.bad_pt, 1, True))


def run_msg(r, off, in_place):
    import torch

    from suruga_amd import msg

    key_t, adt = to_dev(u8(KEY)), to_dev(u8(MSG_AD))
    for what, inp, want, st_want, keep in msg_cases(r):
        what = f"{what} n={r.n} offset={off} in_place={in_place}"
        room = max(len(inp), len(want))
        size = 2 * M + off + room
        if in_place:
            # what the input leaves behind the output (an opened message: its 16 tag bytes) stays
            parts = [(M + off, inp), (M + off, want)]
            salt, tries = fp.pick_salt(size, parts, 0x41)
            d_out = to_dev(fp.image(size, salt, [(M + off, inp)]))
            d_in = d_out[M + off:]
        else:
            parts = [(M + off, want)]
            salt, tries = fp.pick_salt(size, parts, 0x41)
            d_out = to_dev(fp.sentinel(size, salt))
            in_img = fp.image(2 * M + len(inp) + 1, 0x7A, [(M, inp)])
            d_whole = to_dev(in_img)
            d_in = d_whole[M:]
        assert tries <= fp.MAX_SALT_TRIES
        out_img = fp.image(size, salt, parts)
        if st_want is None:
            msg.seal_msg(key_t, r.nonce, d_in, d_out[M + off:], ad=adt, in_len=len(inp), stream=0)
        else:
            d_st = to_dev(fp.sentinel(1 + STATUS_PAD, 0x51))
            assert msg.open_(key_t, r.nonce, d_in, d_out[M + off:], d_st, ad=adt, in_len=len(inp), keep_failed=keep,
                             stream=0) == SG_OK, what
            st = host(d_st)
            assert st[0] == st_want, (what, int(st[0]))
            assert np.array_equal(st[1:], fp.sentinel(1 + STATUS_PAD, 0x51)[1:]), f"{what}: status past its byte"
        torch.cuda.synchronize()
        assert (d := fp.first_diff(host(d_out), out_img, [(M + off, M + off + len(want))])) is None, f"{what}: {d}"
        if not in_place:
            assert (d := fp.first_diff(host(d_whole), in_img)) is None, f"{what}: input changed, {d}"


@pytest.mark.parametrize("g", [1, 3, 0])
def test_long_message_device_form(gpu, oracle, groups, g):
    """out at byte offsets 0, 1, 3 and 15 between 256-byte margins, lengths around one
    and two tiles and below two blocks; also in place (out == in), where the 16 tag
    bytes behind an opened plaintext stay as they were."""
    groups(g)
    for n in msg_lengths():
        r = msg_rec(oracle, n)
        for off in MSG_OFFSETS:
            run_msg(r, off, False)
        for off in (0, 3):
            run_msg(r, off, True)


def test_long_message_short_input_touches_nothing(gpu):
    import torch

    from suruga_amd import msg

    key_t = to_dev(u8(KEY))
    d_in, d_out = to_dev(fp.sentinel(64, 1)), to_dev(fp.sentinel(2 * M + 32, 2))
    d_st = to_dev(fp.sentinel(1 + STATUS_PAD, 0x51))
    for n in (0, 1, 15):
        assert msg.open_(key_t, bytes(8), d_in, d_out[M + 1:], d_st, in_len=n, stream=0) == SG_E_SHORT
    torch.cuda.synchronize()
    assert np.array_equal(host(d_out), fp.sentinel(2 * M + 32, 2))
    assert np.array_equal(host(d_st), fp.sentinel(1 + STATUS_PAD, 0x51))


# ---------------------------------------------------------------------------
# host forms: the single-record trait and the long message over host pointers
# ---------------------------------------------------------------------------
HOST_MARGIN = 64
HOST_LENGTHS = (0, 1, 1000, 16384, 32769)
SG_MAX_RECORD_LEN = 32768


def run_host(gpu, oracle, seal_fn, open_fn, enc, dec, n, off):
    rng = np.random.default_rng([n, off, 5])
    pt, nonce, ad = rng.bytes(n), rng.bytes(8), rng.bytes(13)
    sealed = oracle.seal(KEY, nonce, pt, ad)
    bad = bytearray(sealed)
    bad[(n * 3) % len(bad)] ^= 0x04
    u8p = C.POINTER(C.c_uint8)
    for what, fn, ctx, inp, want, rc_want in (("seal", seal_fn, enc, pt, sealed, SG_OK),
                                              ("open", open_fn, dec, sealed, pt, SG_OK),
                                              ("open tampered", open_fn, dec, bytes(bad), bytes(n), SG_E_BAD_MAC)):
        what = f"{what} n={n} offset={off}"
        size = 2 * HOST_MARGIN + off + len(want)
        parts = [(HOST_MARGIN + off, want)]
        salt, tries = fp.pick_salt(size, parts, 0x61)
        assert tries <= fp.MAX_SALT_TRIES
        buf = (C.c_uint8 * size).from_buffer_copy(fp.sentinel(size, salt).tobytes())
        out = C.cast(C.addressof(buf) + HOST_MARGIN + off, u8p)
        assert fn(ctx, nonce, 8, inp, len(inp), ad, len(ad), out) == rc_want, what
        got = np.frombuffer(bytes(buf), dtype=np.uint8)
        assert (d := fp.first_diff(got, fp.image(size, salt, parts),
                                   [(HOST_MARGIN + off, HOST_MARGIN + off + len(want))])) is None, f"{what}: {d}"


@pytest.mark.parametrize("form", ["record", "message"])
def test_host_forms(gpu, oracle, form):
    """sg_seal / sg_open and sg_seal_msg / sg_open_msg into a host buffer with 64-byte
    sentinel margins, the pointer at offsets 0, 1 and 3."""
    from suruga_amd import ChaCha20Poly1305

    aead = ChaCha20Poly1305()
    enc, dec = aead.new_encryptor(KEY), aead.new_decryptor(KEY)
    fns = (gpu.sg_seal, gpu.sg_open) if form == "record" else (gpu.sg_seal_msg, gpu.sg_open_msg)
    for n in HOST_LENGTHS:
        if form == "record" and n > SG_MAX_RECORD_LEN:
            continue  # above the single-record bound: the message form's case
        for off in (0, 1, 3):
            run_host(gpu, oracle, fns[0], fns[1], enc._ptr, dec._ptr, n, off)
