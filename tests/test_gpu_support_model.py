"""The shared checkers of tests/gpu_support.py, seen to fail (CPU only).

check_sealed and check_opened carry most of the GPU suite's assertions, so here
they judge the oracle's own output laid out by two small cases -- which must
pass -- and then the same images with one byte or one status changed, each of
which must raise.  slots() is held against the formulas the tests wrote out
before it existed, and the switch context manager against a stand-in library.
footprint.Outcome.check, the one check of every whole-buffer run, judges numpy
images of a run that went right and then each way such a run can go wrong.
"""
from __future__ import annotations

import numpy as np
import pytest

import footprint as fp
import gpu_support as G


def listed_case(oracle):
    """Lengths 0, 1, 64, 100, 4160 in 16-byte slots, two keys, sequence numbers up to 2^64 - 1."""
    rng = np.random.default_rng(1)
    lens = np.array([0, 1, 64, 100, 4160], dtype=np.uint32)
    in_off, out_off, pt_bytes, ct_bytes = G.slots(lens, 16)
    seqs = np.array([0, 2**64 - 1, 2**32, 7, 2**63], dtype=np.uint64)
    case = G.BatchCase(lens, rng.bytes(pt_bytes), rng.bytes(64), in_off=in_off, out_off=out_off,
                       kidx=np.array([0, 1, 1, 0, 1], dtype=np.uint32), seqs=seqs)
    return case, pt_bytes, ct_bytes


def uniform_case(oracle):
    """Explicit mode: 3 records of 100 bytes at stride 128, 5 bytes of AD."""
    rng = np.random.default_rng(2)
    case = G.BatchCase(np.full(3, 100), rng.bytes(3 * 128), strides=(128, 128), nonces_h=rng.bytes(24),
                       ads_h=rng.bytes(15), adlen=5)
    return case, 3 * 128, 3 * 128


CASES = {"listed": listed_case, "uniform": uniform_case}


@pytest.fixture(params=sorted(CASES))
def built(request, oracle):
    case, pt_bytes, ct_bytes = CASES[request.param](oracle)
    return case, bytes(case.sealed_image(oracle, ct_bytes)), pt_bytes


def flipped(img: bytes, at: int, mask: int = 0x04) -> bytes:
    return G.xor_at(img, at, mask)


def test_the_oracles_own_image_passes(built, oracle):
    case, sealed, pt_bytes = built
    G.check_sealed(case, oracle, sealed)
    G.check_sealed(case, oracle, np.frombuffer(sealed, dtype=np.uint8))
    G.check_opened(case, case.pt_h, bytes(case.count), bytes(case.count), keep=False)
    for i in range(case.count):  # and it is the reference's image: every record opens
        nonce, ad = case.nonce_ad(oracle, i)
        lo, hi = case.out_range(i)
        assert oracle.open(case.key(i), nonce, sealed[lo:hi], ad) == (0, case.pt(i))


def test_check_sealed_sees_one_bit_anywhere_in_a_record(built, oracle):
    case, sealed, _ = built
    last = case.count - 1
    lo, hi = case.out_range(last)
    spots = {"a ciphertext byte": lo + 10, "a tag byte": hi - 16 + 3, "the record's first byte": lo,
             "the record's last byte": hi - 1, "the first record's first byte": case.out_range(0)[0],
             "the first record's last byte": case.out_range(0)[1] - 1}
    for what, at in spots.items():
        for mask in (0x01, 0x80):
            with pytest.raises(AssertionError):
                G.check_sealed(case, oracle, flipped(sealed, at, mask), where=(what,))
    G.check_sealed(case, oracle, flipped(sealed, lo, 1), records=range(last))  # a listed subset looks at nothing else


def test_check_sealed_sees_the_tag_of_an_empty_record(oracle):
    case, _, ct_bytes = listed_case(oracle)
    sealed = bytes(case.sealed_image(oracle, ct_bytes))
    assert case.n(0) == 0
    lo, hi = case.out_range(0)
    assert hi - lo == 16
    for at in (lo, hi - 1):
        with pytest.raises(AssertionError):
            G.check_sealed(case, oracle, flipped(sealed, at))


def test_check_opened_sees_statuses_and_outputs(built, oracle):
    case, _, pt_bytes = built
    count, failed = case.count, case.count - 2
    ok, o, n = bytes(count), int(case.in_off[failed]), case.n(failed)
    back = bytes(case.pt_h)
    for i in range(count):  # a wrong status byte, either way
        for v in (1, 2, 3, 0xFF):
            st = bytearray(count)
            st[i] = v
            with pytest.raises(AssertionError):
                G.check_opened(case, back, bytes(st), ok, keep=False)
            with pytest.raises(AssertionError):
                G.check_opened(case, back, ok, bytes(st), keep=False)
    with pytest.raises(AssertionError):  # a status array that is too short
        G.check_opened(case, back, ok[:-1], ok, keep=False)
    # one record failed: zero-filled without keep
    exp_st = bytearray(count)
    exp_st[failed] = 1
    zeroed = back[:o] + bytes(n) + back[o + n:]
    G.check_opened(case, zeroed, exp_st, exp_st, keep=False)
    for at in (o, o + n // 2, o + n - 1):  # a non-zero byte in it
        with pytest.raises(AssertionError):
            G.check_opened(case, flipped(zeroed, at), exp_st, exp_st, keep=False)
    with pytest.raises(AssertionError):  # its plaintext left in place
        G.check_opened(case, back, exp_st, exp_st, keep=False)
    for nb in (failed - 1, failed + 1):  # a wrong plaintext byte in the intact records beside it
        p, m = int(case.in_off[nb]), case.n(nb)
        for at in (p, p + m - 1):
            with pytest.raises(AssertionError):
                G.check_opened(case, flipped(zeroed, at), exp_st, exp_st, keep=False)
    # keep: the caller's decryption where it gives one, else anything
    kept = {failed: G.xor_at(case.pt(failed), 0, 0x40)}
    kept_img = flipped(back, o, 0x40)
    G.check_opened(case, kept_img, exp_st, exp_st, keep=True, expect_pt=kept)
    G.check_opened(case, zeroed, exp_st, exp_st, keep=True)
    for img in (back, zeroed, flipped(kept_img, o + n - 1)):
        with pytest.raises(AssertionError):
            G.check_opened(case, img, exp_st, exp_st, keep=True, expect_pt=kept)
    # status 2 / 3: untouched where the caller names the fill
    exp_st[failed] = 3
    ee = back[:o] + b"\xee" * n + back[o + n:]
    G.check_opened(case, ee, exp_st, exp_st, keep=False, fill=0xEE)
    G.check_opened(case, zeroed, exp_st, exp_st, keep=False)
    with pytest.raises(AssertionError):
        G.check_opened(case, flipped(ee, o + 1), exp_st, exp_st, keep=False, fill=0xEE)


WHOLE_LENS = (5, 16, 33)
WHOLE_ST, WHOLE_CL = (0, 1, 2), (5, 16, 70000)


def whole_outcome():
    """The images of an open of three records that did everything right: output between
    margins and gaps, input, a status array and a uint32 content_len array with tails."""
    off, _, size, _ = fp.layout(WHOLE_LENS, WHOLE_LENS)
    want = fp.image(size, 0x21, [(o, bytes([0xC0 + i]) * n) for i, (o, n) in enumerate(zip(off, WHOLE_LENS))])
    inp = fp.sentinel(300, 0x22)
    st0, cl0 = fp.array_start(3, 0x51), fp.array_start(3, 0x53, np.uint32)
    st, cl = st0.copy(), cl0.copy()
    st[:3], cl[:3] = WHOLE_ST, WHOLE_CL
    o = fp.Outcome(want.copy(), want, fp.ranges(off, WHOLE_LENS), inp.copy(), inp,
                   arrays={"status": fp.Array(st, st0), "content_len": fp.Array(cl, cl0)})
    return o, [int(x) for x in off]


def test_whole_buffer_check_passes_on_the_right_images():
    o, _ = whole_outcome()
    o.check(WHOLE_ST, WHOLE_CL, where=("right",))
    assert len(o.arrays["status"].got) == 3 + fp.ARRAY_PAD and o.arrays["content_len"].got.dtype == np.uint32


WHOLE_FAULTS = {
    "a wrong byte inside a record": (lambda o, off: o.out.__setitem__(off[1] + 3, o.out[off[1] + 3] ^ 1), "output", "record 1 byte 3 of 16"),
    "a record's last byte": (lambda o, off: o.out.__setitem__(off[2] + 32, 0), "output", "record 2 byte 32 of 33"),
    "a byte written just behind a record": (lambda o, off: o.out.__setitem__(off[1] + 16, o.out[off[1] + 16] ^ 0x80), "output",
                                            "1 bytes before record 2, 0 behind record 1"),
    "a byte behind the last record": (lambda o, off: o.out.__setitem__(off[2] + 33, o.out[off[2] + 33] ^ 1), "output",
                                      "0 bytes behind the last record"),
    "a byte in the front margin": (lambda o, off: o.out.__setitem__(0, o.out[0] ^ 1), "output", "before record 0"),
    "a changed input byte": (lambda o, off: o.inp.__setitem__(299, o.inp[299] ^ 4), "input", "byte 299"),
    "a wrong status": (lambda o, off: o.arrays["status"].got.__setitem__(1, 0), "status", None),
    "a wrong content_len": (lambda o, off: o.arrays["content_len"].got.__setitem__(2, 70000 & 0xFFFF), "content_len", None),
    "the byte behind the statuses": (lambda o, off: o.arrays["status"].got.__setitem__(3, 0), "status tail", None),
    "the last entry of an array's tail": (lambda o, off: o.arrays["content_len"].got.__setitem__(3 + fp.ARRAY_PAD - 1, 0),
                                          "content_len tail", None),
}


@pytest.mark.parametrize("fault", sorted(WHOLE_FAULTS))
def test_whole_buffer_check_sees(fault):
    spoil, label, detail = WHOLE_FAULTS[fault]
    o, off = whole_outcome()
    spoil(o, off)
    with pytest.raises(AssertionError) as e:
        o.check(WHOLE_ST, WHOLE_CL, where=("ctx", 7))
    msg = e.value.args[0]
    assert msg[:3] == ("ctx", 7, label), msg  # the caller's context, then which comparison
    assert detail is None or detail in msg[3], msg


def test_whole_buffer_check_wants_an_array_without_values_untouched():
    """A seal hands check() no statuses: then the status array must be as uploaded."""
    o, _ = whole_outcome()
    with pytest.raises(AssertionError) as e:
        o.check(where=("seal",))
    assert e.value.args[0][:2] == ("seal", "status tail")
    with pytest.raises(AssertionError) as e:
        o.check(WHOLE_ST, where=("no lengths",))
    assert e.value.args[0][:2] == ("no lengths", "content_len tail")
    with pytest.raises(AssertionError):  # more values than the run has arrays
        o.check(WHOLE_ST, WHOLE_CL, WHOLE_ST)
    o.arrays = {}
    o.check(where=("no arrays",))


@pytest.mark.parametrize("align,skew", [(16, (0, 0)), (1, (0, 0)), (16, (3, 5)), (1, (3, 7))])
def test_slots_are_the_formulas_the_tests_wrote_out(align, skew):
    rng = np.random.default_rng(3)
    lens = rng.integers(0, 16385, size=200).astype(np.uint32)
    lens[:6] = [0, 1, 15, 16, 17, 16384]
    # as in test_gpu_parity / test_gpu_fuzz / test_gpu_concurrency before gpu_support.slots
    pad = align
    step_i = ((lens.astype(np.uint64) + pad - 1) // pad) * pad + skew[0]
    step_o = ((lens.astype(np.uint64) + 16 + pad - 1) // pad) * pad + skew[1]
    in_off = np.zeros(len(lens), dtype=np.uint64)
    out_off = np.zeros(len(lens), dtype=np.uint64)
    in_off[1:] = np.cumsum(step_i[:-1])
    out_off[1:] = np.cumsum(step_o[:-1])
    got = G.slots(lens, align, skew)
    assert got[0].dtype == np.uint64 and got[1].dtype == np.uint64
    assert np.array_equal(got[0], in_off) and np.array_equal(got[1], out_off)
    assert got[2:] == (int(in_off[-1] + step_i[-1]), int(out_off[-1] + step_o[-1]))
    if align == 16 and skew == (0, 0):  # and test_gpu_mac_edges' form of the same offsets
        l64 = lens.astype(np.uint64)
        assert np.array_equal(got[0][1:], np.cumsum((l64 + 15) // 16 * 16)[:-1])
        assert np.array_equal(got[1][1:], np.cumsum((l64 + 16 + 15) // 16 * 16)[:-1])


class FakeLib:
    START = {"sg_set_lockstep": 1, "sg_set_packed": 1, "sg_set_msg_groups": 0, "sg_set_tls13_buckets": 0}

    def __init__(self):
        self.v = dict(self.START)
        self.stuck = None

    def __getattr__(self, name):
        def setter(x):
            prev = self.v[name]
            if x >= 0 and name != self.stuck:
                self.v[name] = x
            return prev
        return setter


def test_kernel_forms_set_check_and_restore():
    lib = FakeLib()
    assert set(G.SWITCHES.values()) == set(lib.START)
    with G.kernel_forms(lib, lockstep=0, groups=3, tls13_buckets=1):
        assert lib.v == {"sg_set_lockstep": 0, "sg_set_packed": 1, "sg_set_msg_groups": 3, "sg_set_tls13_buckets": 1}
        with G.kernel_forms(lib, lockstep=1, tls13_buckets=0):
            assert lib.v["sg_set_lockstep"] == 1 and lib.v["sg_set_tls13_buckets"] == 0
        assert lib.v["sg_set_lockstep"] == 0 and lib.v["sg_set_tls13_buckets"] == 1
    assert lib.v == lib.START
    with pytest.raises(RuntimeError):  # restored when the body raises
        with G.kernel_forms(lib, packed=0, tls13_buckets=1):
            raise RuntimeError
    assert lib.v["sg_set_packed"] == 1 and lib.v["sg_set_tls13_buckets"] == 0
    for stuck in ("sg_set_packed", "sg_set_tls13_buckets"):
        lib.stuck = stuck  # a switch that does not take: the readback fails, the others are put back
        with pytest.raises(AssertionError):
            with G.kernel_forms(lib, lockstep=0, packed=0, tls13_buckets=1):
                pass
        assert lib.v == lib.START, stuck


def test_support_module_needs_no_torch():
    """Imported here without torch: a CPU-only process can use the checkers."""
    import subprocess
    import sys
    from pathlib import Path

    code = ("import sys; sys.modules['torch'] = None; sys.path.insert(0, sys.argv[1]); import gpu_support; "
            "assert gpu_support.slots([1, 2], 16)[2] == 32")
    subprocess.run([sys.executable, "-c", code, str(Path(__file__).parent)], check=True, timeout=60)
