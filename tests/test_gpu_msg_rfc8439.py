"""GPU parity of the message path in RFC 8439 (SG_MSG_RFC8439 on
sg_seal_msg_dev / sg_open_msg_dev, sg_seal_msg_rfc8439 / sg_open_msg_rfc8439 on
host memory, the ChaCha20Poly1305Rfc8439 mirror): every byte against
tests/rfc8439_ref.py, which tests/test_rfc8439_ref.py ties to OpenSSL.

Every device call here runs on sentinel buffers (tests/footprint.py) and the
whole buffers are compared afterwards: a seal writes exactly n + 16 bytes, an
open exactly n, and neither touches its input or the AD.

T below is the plan's tile_bytes.  The shapes (rfc8439_ref.single_shapes) put
the AD's padding, the ciphertext's padding and the length block just before,
on and just behind the edges of one, two and three tiles."""
from __future__ import annotations

import ctypes as C
import hashlib

import numpy as np
import pytest

import footprint as fp
import rfc8439_ref as ref
from gpu_support import groups, host_np  # noqa: F401  (groups: a fixture)
from suruga_amd._native import SG_E_BAD_MAC, SG_E_SHORT, SG_OK

pytestmark = pytest.mark.gpu

T = ref.TB
UNALIGNED_SHAPES = [(65, 17), (2 * T - 33, 13), (100, T + 1)]  # (n, adlen): small, ct edge, AD across a tile
OFFSETS = (1, 7, 15)


@pytest.fixture(scope="module")
def key_t(gpu):
    import torch

    return torch.tensor(list(ref.KEY), dtype=torch.uint8, device="cuda")


class Buf:
    """`room` bytes `off` past a 16-byte boundary inside a sentinel buffer, `content` at their start."""

    def __init__(self, content: bytes, off: int, room: int, salt: int):
        import torch

        self.lo = fp.MARGIN + off
        self.size = fp.round_up(self.lo + room, 16) + fp.MARGIN
        self.salt, self.room = salt, room
        self.t = torch.from_numpy(fp.image(self.size, salt, [(self.lo, content)])).cuda()
        assert self.t.data_ptr() % 16 == 0
        self.view = self.t[self.lo:self.lo + room]  # (the message calls take an AD's length from its tensor)

    def check(self, content: bytes, what):
        d = fp.first_diff(host_np(self.t), fp.image(self.size, self.salt, [(self.lo, content)]),
                          [(self.lo, self.lo + self.room)])
        assert d is None, (what, d)


def salt_for(room: int, off: int, content: bytes, first: int) -> int:
    """A salt under which the content's first and last byte differ from the sentinel under them."""
    lo = fp.MARGIN + off
    return fp.pick_salt(fp.round_up(lo + room, 16) + fp.MARGIN, [(lo, content)], first)[0]


def seal_dev(key_t, pt: bytes, ad: bytes, want: bytes, *, nonce=ref.NONCE, offs=(0, 0, 0), in_place=False, where=()):
    """One sg_seal_msg_dev with SG_MSG_RFC8439; every buffer is checked whole."""
    from suruga_amd import msg

    n = len(pt)
    adb = Buf(ad, offs[2], len(ad), 0x31)
    if in_place:
        io = Buf(pt, offs[0], n + 16, salt_for(n + 16, offs[0], want, 0x11))
        msg.seal_msg(key_t, nonce, io.view, io.view, ad=adb.view, in_len=n, stream=0, rfc8439=True)
        io.check(want, (*where, "seal in place"))
    else:
        inb = Buf(pt, offs[0], n, 0x21)
        out = Buf(b"", offs[1], n + 16, salt_for(n + 16, offs[1], want, 0x11))
        msg.seal_msg(key_t, nonce, inb.view, out.view, ad=adb.view, in_len=n, stream=0, rfc8439=True)
        out.check(want, (*where, "seal out"))
        inb.check(pt, (*where, "seal in"))
    adb.check(ad, (*where, "seal ad"))


def open_dev(key_t, sealed: bytes, ad: bytes, want_st: int, want: bytes | None, *, nonce=ref.NONCE, offs=(0, 0, 0),
             in_place=False, keep_failed=False, where=()):
    """One sg_open_msg_dev with SG_MSG_RFC8439: the status and every buffer, whole.
    want: the n bytes the output range must hold (None: untouched)."""
    import torch

    from suruga_amd import msg

    n = len(sealed) - 16
    adb = Buf(ad, offs[2], len(ad), 0x32)
    st = torch.full((65,), 0xFF, dtype=torch.uint8, device="cuda")
    if in_place:
        after = sealed if want is None else want + sealed[n:]  # the tag behind the plaintext is left alone
        io = Buf(sealed, offs[0], n + 16, 0x12)
        rc = msg.open_(key_t, nonce, io.view, io.view, st, ad=adb.view, in_len=n + 16, keep_failed=keep_failed,
                       stream=0, rfc8439=True)
        io.check(after, (*where, "open in place"))
    else:
        inb = Buf(sealed, offs[0], n + 16, 0x22)
        out = Buf(b"", offs[1], n, salt_for(n, offs[1], want, 0x12) if want else 0x12)
        rc = msg.open_(key_t, nonce, inb.view, out.view, st, ad=adb.view, in_len=n + 16, keep_failed=keep_failed,
                       stream=0, rfc8439=True)
        out.check(b"" if want is None else want, (*where, "open out"))
        inb.check(sealed, (*where, "open in"))
    adb.check(ad, (*where, "open ad"))
    st_h = host_np(st)
    assert rc == SG_OK and int(st_h[0]) == want_st and (st_h[1:] == 0xFF).all(), (*where, rc, st_h[:2])


@pytest.mark.parametrize("g", [1, 2, 0])
def test_every_shape_device_form(gpu, key_t, groups, g):
    groups(g)
    for n, adlen in ref.single_shapes():
        _, _, pt, ad = ref.single_message(n, adlen)
        want = ref.sealed_single(n, adlen)
        seal_dev(key_t, pt, ad, want, where=(g, n, adlen))
        open_dev(key_t, want, ad, SG_OK, pt, where=(g, n, adlen))


@pytest.mark.parametrize("g", [1, 2, 0])
def test_misaligned_and_in_place(gpu, key_t, groups, g):
    """in, out and ad 1, 7 and 15 bytes off a 16-byte boundary, apart and in place."""
    groups(g)
    for n, adlen in UNALIGNED_SHAPES:
        _, _, pt, ad = ref.single_message(n, adlen)
        want = ref.sealed_single(n, adlen)
        for k, off in enumerate(OFFSETS):
            offs = (off, OFFSETS[(k + 1) % 3], OFFSETS[(k + 2) % 3])
            seal_dev(key_t, pt, ad, want, offs=offs, where=(n, adlen, offs))
            open_dev(key_t, want, ad, SG_OK, pt, offs=offs, where=(n, adlen, offs))
            seal_dev(key_t, pt, ad, want, offs=(off, off, off), in_place=True, where=(n, adlen, off))
            open_dev(key_t, want, ad, SG_OK, pt, offs=(off, off, off), in_place=True, where=(n, adlen, off))
        # aligned in and out with the AD alone off the boundary, and the reverse
        seal_dev(key_t, pt, ad, want, offs=(0, 0, 7), where=(n, adlen, "ad"))
        open_dev(key_t, want, ad, SG_OK, pt, offs=(7, 7, 0), where=(n, adlen, "in, out"))


def test_nonce_hi_is_state_word_13(gpu, oracle, key_t):
    """Four different bytes in nonce_hi; one flipped bit changes ciphertext and tag;
    without the flag the field is never read."""
    from suruga_amd import _native as N
    from suruga_amd import msg

    n, adlen = T + 100, 13
    _, _, pt, ad = ref.single_message(n, adlen)
    assert len(set(ref.NONCE[:4])) == 4
    base = ref.sealed_single(n, adlen)
    seal_dev(key_t, pt, ad, base)
    for byte in range(4):
        nonce = bytearray(ref.NONCE)
        nonce[byte] ^= 1 << (2 * byte + 1)
        want = ref.seal(ref.KEY, bytes(nonce), pt, ad)
        assert want[:64] != base[:64] and want[n:] != base[n:]
        assert sum(a != b for a, b in zip(want[:n], base[:n])) > n * 0.99  # another keystream
        seal_dev(key_t, pt, ad, want, nonce=bytes(nonce), where=("nonce_hi byte", byte))
        open_dev(key_t, want, ad, SG_OK, pt, nonce=bytes(nonce), where=("nonce_hi byte", byte))
        open_dev(key_t, base, ad, SG_E_BAD_MAC, bytes(n), nonce=bytes(nonce), where=("wrong nonce_hi", byte))
    # flag off: garbage in nonce_hi, and the draft's bytes come out
    import torch

    nonce8 = ref.NONCE[4:]
    want = oracle.seal(ref.KEY, nonce8, pt, ad)
    inb, adb = Buf(pt, 0, n, 0x21), Buf(ad, 0, adlen, 0x31)
    for garbage in (bytes(4), b"\xff" * 4, ref.NONCE[:4]):
        out = Buf(b"", 0, n + 16, 0x11)
        m = msg._msg(key_t, nonce8, adb.view, inp=inb.view, in_len=n, out=out.view, status=None, keep_failed=False,
                     stream=0, workspace=None)
        m.nonce_hi[:] = garbage
        assert m.flags == 0 and gpu.sg_seal_msg_dev(C.byref(m)) == SG_OK
        torch.cuda.synchronize()
        out.check(want, ("draft with garbage in nonce_hi", garbage))
        st = torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")
        back = Buf(b"", 0, n, 0x12)
        m = msg._msg(key_t, nonce8, adb.view, inp=out.view, in_len=n + 16, out=back.view, status=st, keep_failed=False,
                     stream=0, workspace=None)
        m.nonce_hi[:] = garbage
        assert gpu.sg_open_msg_dev(C.byref(m)) == SG_OK
        torch.cuda.synchronize()
        assert int(st.item()) == SG_OK
        back.check(pt, ("draft open with garbage in nonce_hi", garbage))


@pytest.mark.parametrize("n,adlen", [(17, 13), (2 * T - 33, 13), (2 * T + 5, T - 15)])
def test_open_tamper(gpu, key_t, n, adlen):
    """One flipped bit anywhere is SG_E_BAD_MAC; the output is zeroed, or with
    SG_MSG_KEEP_FAILED the decryption that always runs."""
    _, _, pt, ad = ref.single_message(n, adlen)
    sealed = ref.sealed_single(n, adlen)
    flips = [("first", 0), ("middle", n // 2), ("last", n - 1)] + [(f"tag byte {i}", n + i) for i in range(16)]
    for k, (where, at) in enumerate(flips):
        bad = bytearray(sealed)
        bad[at] ^= 1 << (k % 8)
        bad = bytes(bad)
        rc, plain = ref.open(ref.KEY, ref.NONCE, bad, ad)
        assert rc == SG_E_BAD_MAC
        open_dev(key_t, bad, ad, SG_E_BAD_MAC, bytes(n), where=(where,))
        open_dev(key_t, bad, ad, SG_E_BAD_MAC, plain, keep_failed=True, where=(where, "keep"))
    for at in (0, adlen // 2, adlen - 1):
        bad_ad = bytearray(ad)
        bad_ad[at] ^= 0x10
        open_dev(key_t, sealed, bytes(bad_ad), SG_E_BAD_MAC, bytes(n), offs=(0, 3, 0), where=("ad", at))
        open_dev(key_t, sealed, bytes(bad_ad), SG_E_BAD_MAC, pt, keep_failed=True, where=("ad", at, "keep"))
    open_dev(key_t, sealed, ad, SG_E_BAD_MAC, bytes(n), in_place=True, nonce=ref.NONCE[:11] + b"\0",
             where=("nonce, in place",))


def test_padding_forgery(gpu, key_t):
    """ad with one zero byte more (or one fewer) under the same ciphertext and tag
    is another message: the padded bytes are the same, the length block is not."""
    for n, adlen in [(17, 0), (17, 1), (64, 13), (65, 15), (16, 16), (100, T - 17), (100, T - 16), (1, T - 1)]:
        key, nonce, pt, _ = ref.single_message(n, adlen)
        ad = ref.data(adlen, b"forgery ad %d" % adlen)
        sealed = ref.seal(key, nonce, pt, ad)
        longer = ad + b"\0"
        if adlen % 16:
            assert ref.mac_stream(longer, sealed[:n])[:-16] == ref.mac_stream(ad, sealed[:n])[:-16]
        open_dev(key_t, sealed, ad, SG_OK, pt, where=(n, adlen))
        open_dev(key_t, sealed, longer, SG_E_BAD_MAC, bytes(n), where=(n, adlen, "ad + 00"))
        sealed0 = ref.seal(key, nonce, pt, longer)
        open_dev(key_t, sealed0, longer, SG_OK, pt, where=(n, adlen, "sealed with ad + 00"))
        open_dev(key_t, sealed0, ad, SG_E_BAD_MAC, bytes(n), where=(n, adlen, "ad - 00"))
    # the same on the data side: a ciphertext one zero byte longer under the same tag
    key, nonce, pt, ad = ref.single_message(17, 13)
    sealed = ref.sealed_single(17, 13)
    grown = sealed[:17] + b"\0" + sealed[17:]
    open_dev(key_t, grown, ad, SG_E_BAD_MAC, bytes(18), where=("ct + 00",))


def test_short_input(gpu, key_t):
    import torch

    from suruga_amd import msg

    st = torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")
    inb, out = Buf(bytes(15), 0, 15, 0x22), Buf(b"", 0, 16, 0x12)
    assert msg.open_(key_t, ref.NONCE, inb.view, out.view, st, in_len=15, stream=0, rfc8439=True) == SG_E_SHORT
    torch.cuda.synchronize()
    assert int(st.item()) == 0xFF
    out.check(b"", "short open")


def test_host_forms_reproduce_the_stored_vectors(gpu):
    """OpenSSL's own outputs (tests/golden/rfc8439_vectors.json), full vectors."""
    from suruga_amd import ChaCha20Poly1305Rfc8439, TlsError, TlsErrorKind

    gold = ref.golden()
    aead = ChaCha20Poly1305Rfc8439()
    assert len(gold["small"]) == 64
    ctx = {}
    for v in gold["small"]:
        key, nonce, pt, ad, want = (bytes.fromhex(v[f]) for f in ("key", "nonce", "pt", "ad", "ct_tag"))
        if key not in ctx:
            ctx[key] = (aead.new_encryptor(key), aead.new_decryptor(key))
        enc, dec = ctx[key]
        n = len(pt)
        out = (C.c_uint8 * (n + 16))()
        assert gpu.sg_seal_msg_rfc8439(enc._ptr, nonce, 12, pt, n, ad, len(ad), out) == SG_OK, (n, len(ad))
        assert bytes(out) == want, (n, len(ad))
        back = (C.c_uint8 * max(n, 1))()
        assert gpu.sg_open_msg_rfc8439(dec._ptr, nonce, 12, want, n + 16, ad, len(ad), back) == SG_OK, (n, len(ad))
        assert bytes(back)[:n] == pt
        assert enc.encrypt(nonce, pt, ad) == want and dec.decrypt(nonce, want, ad) == pt
        bad = bytearray(want)
        bad[-1] ^= 0x80
        back = (C.c_uint8 * max(n, 1))(*([0xEE] * max(n, 1)))
        assert gpu.sg_open_msg_rfc8439(dec._ptr, nonce, 12, bytes(bad), n + 16, ad, len(ad), back) == SG_E_BAD_MAC
        assert bytes(back)[:n] == bytes(n)
        with pytest.raises(TlsError) as e:
            dec.decrypt(nonce, bytes(bad), ad)
        assert e.value.kind is TlsErrorKind.BadRecordMac and e.value.desc == "wrong mac"
    with pytest.raises(TlsError) as e:
        dec.decrypt(nonce, bytes(15), b"")
    assert e.value.desc == "message too short"
    with pytest.raises(ValueError):
        enc.encrypt(bytes(8), b"", b"")


def test_trait_mirror_round_trip_one_mebibyte_and_seven(gpu):
    from suruga_amd import ChaCha20Poly1305Rfc8439

    n, adlen = (1 << 20) + 7, 13
    stored = [v for v in ref.golden()["shapes"]["single"] if (v["n"], v["adlen"]) == (n, adlen)]
    assert len(stored) == 1
    key, nonce, pt, ad = ref.single_message(n, adlen)
    aead = ChaCha20Poly1305Rfc8439()
    out = aead.new_encryptor(key).encrypt(nonce, pt, ad)
    assert out[n:].hex() == stored[0]["tag"] and hashlib.sha256(out[:n]).hexdigest() == stored[0]["ct_sha256"]
    assert out == ref.sealed_single(n, adlen)
    assert aead.new_decryptor(key).decrypt(nonce, out, ad) == pt


def test_stored_digests_of_the_device_shapes(gpu, key_t):
    """The device form against OpenSSL's digests directly, at the tile-edge shapes."""
    import torch

    from suruga_amd import msg

    stored = {(v["n"], v["adlen"]): v for v in ref.golden()["shapes"]["single"]}
    for n, adlen in ref.ct_edge_shapes() + ref.ad_edge_shapes():
        _, _, pt, ad = ref.single_message(n, adlen)
        inp = torch.from_numpy(np.frombuffer(pt + bytes(16), dtype=np.uint8).copy()).cuda()
        adt = torch.from_numpy(np.frombuffer(ad + bytes(1), dtype=np.uint8).copy()).cuda()
        msg.seal_msg(key_t, ref.NONCE, inp, inp, ad=adt[:adlen], in_len=n, stream=0, rfc8439=True)
        got = host_np(inp).tobytes()
        v = stored[(n, adlen)]
        assert got[n:].hex() == v["tag"] and hashlib.sha256(got[:n]).hexdigest() == v["ct_sha256"], (n, adlen)
