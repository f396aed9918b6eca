"""Adversarial Poly1305 states through every kernel form's MAC finish.

The parity tests feed the kernels random bytes, under which the Poly1305
accumulator is a uniformly random field element: the h >= p select of
canonical(), the second-pass fold of ripple_full(), the full carry chain of
tag_words() (sg_device.h) and the worst-case partial sums of the lane
reductions are never reached.  tests/mac_forge.py builds ciphertext that
reaches them (tests/test_mac_forge.py checks its records against the oracle on
the CPU); here every such record goes through both directions of every
finishing path:

  seal     pt -> every output byte equals oracle.seal
  open     ct || tag -> SG_OK and the plaintext
  bad tag  tag + 1 mod 2^128 -> SG_E_BAD_MAC and a zeroed output

Tier A: the final accumulator == 0..6, 63, 64, 255, 319, 320, p-1..p-5,
  2^128-1, 2^128, 2^129, x + k 2^128, and the values that make the tag 00..00
  (every w_i + s_i carries) and ff..ff.
Tier B: every lane term (size classes, packed kernel, long message) and every
  group partial (long message) == -1, whose representative p - 1 has every
  limb at its maximum, and == 0.
Tier C: constant fills and ciphertext aligned with the signs of the
  wave-per-record kernel's signed digits, which drive its i8 MFMA accumulators
  as far from their 2^24 seed as ciphertext can.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import mac_forge as F
from gpu_support import BatchCase, dev_bytes, filled, host_bytes as host, mode_of, open_, seal, slots
from gpu_support import groups, lockstep, packed  # noqa: F401  (fixtures)
from suruga_amd._native import SG_E_BAD_MAC, SG_OK

pytestmark = pytest.mark.gpu


def bad_tag(sealed: bytes) -> bytes:
    """ct || (tag + 1 mod 2^128)."""
    t = (int.from_bytes(sealed[-16:], "little") + 1) & F.M128
    return sealed[:-16] + t.to_bytes(16, "little")


def recs_of(cases):
    return [F.make(*c) for c in cases]


def first_diff(got: bytes, want: bytes, bounds, recs):
    """The case of the first record whose bytes differ (None: all equal)."""
    if got == want:
        return None
    for (lo, hi), r in zip(bounds, recs):
        if got[lo:hi] != want[lo:hi]:
            return r.case
    return "bytes between the records"


@pytest.fixture(scope="module")
def key_t(gpu):
    return dev_bytes(F.KEY)


# ---------------------------------------------------------------------------
# batch forms
# ---------------------------------------------------------------------------
def check_batch(case, recs, ct_bytes, sealed_of, back_of):
    """Seal, open and open with every tag off by one; whole buffers against the forged
    records' images, so the bytes between the records count too.  sealed_of(parts) lays
    parts out as the sealed image, back_of() is the buffer an open writes into and
    back_of(parts) what it must hold afterwards."""
    count = case.count
    in_b = [(int(o), int(o) + case.n(i)) for i, o in enumerate(case.in_off)]
    out_b = [case.out_range(i) for i in range(count)]
    want = sealed_of([r.want for r in recs])
    assert first_diff(bytes(seal(case, filled(ct_bytes, 0))), want, out_b, recs) is None, "seal"
    for sealed, st_want, pt_want in ((want, bytes(count), back_of([r.pt for r in recs])),
                                     (sealed_of([bad_tag(r.want) for r in recs]), b"\x01" * count,
                                      back_of([bytes(len(r.pt)) for r in recs]))):
        back_h, st_h = open_(case, dev_bytes(sealed), back_of())
        assert st_h == st_want, ("open status", [r.case for r, a, b in zip(recs, st_h, st_want) if a != b][:3])
        assert first_diff(back_h, pt_want, in_b, recs) is None, "open output"


def check_uniform(recs, n, mode):
    """A uniform batch (len = NULL, strides n and n + 16: 16-byte aligned for n = 16384)."""
    count = len(recs)
    assert all(len(r.pt) == n for r in recs)
    case = BatchCase(np.full(count, n), b"".join(r.pt for r in recs), F.KEY, strides=(n, n + 16), **mode_of(recs, mode))
    check_batch(case, recs, count * (n + 16), b"".join,
                lambda parts=None: filled(count * n, 0xEE) if parts is None else b"".join(parts))


def check_mixed(recs):
    """A mixed TLS batch (len array, 16-byte aligned records, per-record sequence numbers)."""
    lens = np.array([len(r.pt) for r in recs], dtype=np.uint64)
    in_off, out_off, _, _ = slots(lens, 16)
    # its own sizes: the last record's slot is not rounded up, 16 spare bytes behind each buffer
    pt_bytes = int(in_off[-1] + lens[-1]) + 16
    ct_bytes = int(out_off[-1] + lens[-1]) + 32

    def lay(parts, offs, size):
        buf = bytearray(size)
        for p, o in zip(parts, offs):
            buf[int(o):int(o) + len(p)] = p
        return bytes(buf)

    def back_of(parts=None):
        # before the open 0xEE in the records and zero between them, so that a zeroed record shows
        if parts is None:
            return dev_bytes(lay([b"\xee" * len(r.pt) for r in recs], in_off, pt_bytes))
        return lay(parts, in_off, pt_bytes)

    case = BatchCase(lens, lay([r.pt for r in recs], in_off, pt_bytes), F.KEY, in_off=in_off, out_off=out_off,
                     **mode_of(recs, "tls"))
    check_batch(case, recs, ct_bytes, lambda parts: lay(parts, out_off, ct_bytes), back_of)


# ---------------------------------------------------------------------------
# the long-message forms
# ---------------------------------------------------------------------------
def dev_room(n: int):
    return filled(max(n, 1), 0xEE)


def check_msg_dev(key_t, r):
    from suruga_amd import msg

    n = len(r.pt)
    adt = dev_bytes(r.ad)
    out = dev_room(n + 16)
    msg.seal_msg(key_t, r.nonce, dev_bytes(r.pt), out, ad=adt, in_len=n, stream=0)
    assert host(out)[:n + 16] == r.want, ("seal", r.case)
    for sealed, st_want, pt_want in ((r.want, SG_OK, r.pt), (bad_tag(r.want), SG_E_BAD_MAC, bytes(n))):
        back = dev_room(n)
        st = filled(1, 0xFF)
        assert msg.open_(key_t, r.nonce, dev_bytes(sealed), back, st, ad=adt, in_len=n + 16, stream=0) == SG_OK
        assert int(st.item()) == st_want, ("open status", r.case)
        assert host(back)[:n] == pt_want, ("open output", r.case)


def check_msg_host(gpu, r):
    from suruga_amd import ChaCha20Poly1305

    aead = ChaCha20Poly1305()
    enc, dec = aead.new_encryptor(r.key), aead.new_decryptor(r.key)
    n = len(r.pt)
    out = (C.c_uint8 * (n + 16))()
    assert gpu.sg_seal_msg(enc._ptr, r.nonce, 8, r.pt, n, r.ad, len(r.ad), out) == SG_OK
    assert bytes(out) == r.want, ("seal", r.case)
    back = (C.c_uint8 * n)(*([0xEE] * 64))
    assert gpu.sg_open_msg(dec._ptr, r.nonce, 8, r.want, n + 16, r.ad, len(r.ad), back) == SG_OK
    assert bytes(back) == r.pt, ("open", r.case)
    back = (C.c_uint8 * n)(*([0xEE] * 64))
    assert gpu.sg_open_msg(dec._ptr, r.nonce, 8, bad_tag(r.want), n + 16, r.ad, len(r.ad), back) == SG_E_BAD_MAC
    assert bytes(back) == bytes(n), ("bad tag", r.case)


# ---------------------------------------------------------------------------
# Tier A
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", F.SC_LENGTHS + (F.WPR_N,))
def test_final_accumulator_size_classes(gpu, lockstep, n):
    """Direct launch of one size class (uniform batch); 16 KiB records with the wave-per-record kernel off."""
    lockstep(0 if n == F.WPR_N else 1)
    for mode in F.SC_MODES:
        check_uniform(recs_of(F.sizeclass_a()[(mode, n)]), n, mode)


@pytest.mark.parametrize("mode", F.WPR_MODES)
def test_final_accumulator_wave_per_record(gpu, lockstep, mode):
    lockstep(1)
    check_uniform(recs_of(F.wpr_a()[(mode, F.WPR_N)]), F.WPR_N, mode)


def test_final_accumulator_wave_per_record_buckets(gpu, lockstep, packed):
    lockstep(1)
    packed(1)
    check_mixed(recs_of(F.bucket_a()))


@pytest.mark.parametrize("form", ["packed", "classes"])
def test_final_accumulator_packed_and_listed_classes(gpu, lockstep, packed, form):
    """More than one 128-record run of the packed list; the same batch with both
    switches off goes through the list-driven size classes."""
    on = 1 if form == "packed" else 0
    lockstep(on)
    packed(on)
    recs = recs_of(F.packed_a())
    assert len(recs) > 128
    check_mixed(recs)


@pytest.mark.parametrize("g", [1, 2, 3, 0])
def test_final_accumulator_long_message_device_form(gpu, key_t, groups, g):
    groups(g)
    for cases in F.msg_a().values():
        for r in recs_of(cases):
            check_msg_dev(key_t, r)


def test_final_accumulator_long_message_host_form(gpu):
    n = F.msg_lengths()[-1]
    for r in recs_of(F.msg_a()[n]):
        check_msg_host(gpu, r)


def test_final_accumulator_single_record_trait(gpu):
    from suruga_amd import ChaCha20Poly1305, TlsError, TlsErrorKind

    aead = ChaCha20Poly1305()
    enc, dec = aead.new_encryptor(F.KEY), aead.new_decryptor(F.KEY)
    for r in recs_of(F.trait_a()):
        assert enc.encrypt(r.nonce, r.pt, r.ad) == r.want, ("seal", r.case)
        assert dec.decrypt(r.nonce, r.want, r.ad) == r.pt, ("open", r.case)
        with pytest.raises(TlsError) as e:
            dec.decrypt(r.nonce, bad_tag(r.want), r.ad)
        assert e.value.kind is TlsErrorKind.BadRecordMac and e.value.desc == "wrong mac", r.case


# ---------------------------------------------------------------------------
# Tier B
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("mode", F.SC_MODES)
def test_lane_terms_size_classes(gpu, lockstep, mode):
    lockstep(1)
    for (m, n), cases in F.sizeclass_b().items():
        if m == mode:
            check_uniform(recs_of(cases), n, mode)


def test_lane_terms_packed(gpu, lockstep, packed):
    lockstep(1)
    packed(1)
    check_mixed(recs_of(F.packed_b()))


@pytest.mark.parametrize("g", F.MSG_GROUPS_B)
def test_lane_terms_and_group_partials_long_message(gpu, key_t, groups, g):
    groups(g)
    for r in recs_of(F.msg_b()[g]):
        check_msg_dev(key_t, r)


# ---------------------------------------------------------------------------
# Tier C
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wpr", "sizeclass"])
def test_mfma_accumulator_extremes(gpu, lockstep, form):
    """Fills and sign-aligned ciphertext through the wave-per-record kernel; the
    same records with lock-step off (size class 7) as the control."""
    lockstep(1 if form == "wpr" else 0)
    check_uniform(recs_of(F.wpr_c()), F.WPR_N, "tls")


def test_fills_through_the_packed_kernel_and_a_size_class(gpu, lockstep, packed):
    lockstep(1)
    packed(1)
    for (mode, n), cases in F.fills_other().items():
        recs = recs_of(cases)
        if n == 4096:
            check_mixed(recs + recs_of(F.packed_b())[:2])  # beside records of another length: len array, class > 0
        else:
            check_uniform(recs, n, mode)
