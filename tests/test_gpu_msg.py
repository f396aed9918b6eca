"""GPU parity of the long-message path (sg_seal_msg_dev / sg_open_msg_dev on
device memory, sg_seal_msg / sg_open_msg on host memory, and the trait mirrors
above the single-record bounds): every byte against oracle.seal / oracle.open.

T below is the plan's tile_bytes; the tile-edge lengths put the end of the MAC
stream ad || le64(adlen) || ct || le64(n) just before, on and just after one,
two and three tiles."""
from __future__ import annotations

import ctypes as C
import functools
import subprocess

import numpy as np
import pytest

from conftest import vector_pt
from gpu_support import groups, host_bytes as host  # noqa: F401  (groups: a fixture)
from mac_forge import tile_bytes
from suruga_amd._native import SG_E_BAD_MAC, SG_E_SHORT, SG_OK

pytestmark = pytest.mark.gpu

KEY = bytes(range(32))
NONCE = bytes([0xA0, 1, 2, 3, 4, 5, 6, 0x7F])


@functools.lru_cache(maxsize=None)
def data(n: int, seed: int = 1) -> bytes:
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


_sealed: dict = {}


def want_sealed(oracle, n: int, adlen: int) -> bytes:
    """oracle.seal of data(n) under data(adlen, 2), computed once per shape."""
    if (n, adlen) not in _sealed:
        _sealed[(n, adlen)] = oracle.seal(KEY, NONCE, data(n), data(adlen, 2))
    return _sealed[(n, adlen)]


def dev(b: bytes, off: int = 0, room: int = 0):
    """b in device memory, its first byte `off` bytes past a 16-byte boundary, `room` spare bytes behind."""
    import torch

    base = torch.zeros(len(b) + room + off + 16, dtype=torch.uint8, device="cuda")
    assert base.data_ptr() % 16 == 0
    t = base[off:off + len(b) + room]
    if b:
        t[:len(b)] = torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()
    return t


@pytest.fixture(scope="module")
def key_t(gpu):
    import torch

    return torch.tensor(list(KEY), dtype=torch.uint8, device="cuda")


def seal_dev(key_t, pt: bytes, ad: bytes, offs=(0, 0, 0), key=None, nonce=NONCE) -> bytes:
    from suruga_amd import msg

    n = len(pt)
    inp, adt = dev(pt, offs[0]), dev(ad, offs[2])
    out = dev(b"", offs[1], room=n + 16)
    msg.seal_msg(key_t if key is None else key, nonce, inp, out, ad=adt, in_len=n, stream=0)
    return host(out)


def open_dev(key_t, ct: bytes, ad: bytes, offs=(0, 0, 0), keep_failed=False, key=None, nonce=NONCE):
    import torch

    from suruga_amd import msg

    n = len(ct) - 16
    inp, adt = dev(ct, offs[0]), dev(ad, offs[2])
    out = dev(b"", offs[1], room=max(n, 1))
    out.fill_(0xEE)
    st = torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")
    rc = msg.open_(key_t if key is None else key, nonce, inp, out, st, ad=adt, in_len=len(ct),
                   keep_failed=keep_failed, stream=0)
    return rc, int(st.item()), host(out)[:n]


def test_small_domain_vectors(gpu, oracle, aead_vectors):
    """Every stored vector (n = 0 with adlen = 0 among them) through the host forms."""
    from suruga_amd import ChaCha20Poly1305

    aead = ChaCha20Poly1305()
    seen_empty = False
    for v in aead_vectors["vectors"]:
        key, nonce, ad = bytes.fromhex(v["key"]), bytes.fromhex(v["nonce"]), bytes.fromhex(v["ad"])
        pt = vector_pt(v, oracle)
        seen_empty |= not pt and not ad
        enc, dec = aead.new_encryptor(key), aead.new_decryptor(key)
        out = (C.c_uint8 * (len(pt) + 16))()
        assert gpu.sg_seal_msg(enc._ptr, nonce, 8, pt, len(pt), ad, len(ad), out) == SG_OK, v["name"]
        assert bytes(out) == oracle.seal(key, nonce, pt, ad), v["name"]
        assert bytes(out)[-16:].hex() == v["tag"], v["name"]
        back = (C.c_uint8 * max(len(pt), 1))()
        assert gpu.sg_open_msg(dec._ptr, nonce, 8, bytes(out), len(pt) + 16, ad, len(ad), back) == SG_OK, v["name"]
        assert bytes(back)[:len(pt)] == pt, v["name"]
    if not seen_empty:
        out = (C.c_uint8 * 16)()
        enc = aead.new_encryptor(KEY)
        assert gpu.sg_seal_msg(enc._ptr, NONCE, 8, b"", 0, b"", 0, out) == SG_OK
        assert bytes(out) == oracle.seal(KEY, NONCE, b"", b"")


@pytest.mark.parametrize("n,adlen", [(100, 256), (100, 1000), (100, 4096), (100, 70001),
                                     (32769, 13), (65536, 13), ((1 << 20) + 7, 13)])
def test_host_form_past_the_old_bounds(gpu, oracle, n, adlen):
    from suruga_amd import ChaCha20Poly1305

    aead = ChaCha20Poly1305()
    enc, dec = aead.new_encryptor(KEY), aead.new_decryptor(KEY)
    pt, ad = data(n), data(adlen, 2)
    out = (C.c_uint8 * (n + 16))()
    assert gpu.sg_seal_msg(enc._ptr, NONCE, 8, pt, n, ad, adlen, out) == SG_OK
    assert bytes(out) == want_sealed(oracle, n, adlen)
    back = (C.c_uint8 * n)()
    assert gpu.sg_open_msg(dec._ptr, NONCE, 8, bytes(out), n + 16, ad, adlen, back) == SG_OK
    assert bytes(back) == pt


@pytest.mark.parametrize("n,adlen", [(32769, 13), (100, 256)])
def test_trait_round_trip_past_the_old_bounds(gpu, oracle, n, adlen):
    """Encryptor.encrypt / Decryptor.decrypt take any length (cipher/mod.rs:22-32)."""
    from suruga_amd import ChaCha20Poly1305, TlsError, TlsErrorKind

    aead = ChaCha20Poly1305()
    pt, ad = data(n), data(adlen, 2)
    out = aead.new_encryptor(KEY).encrypt(NONCE, pt, ad)
    assert out == want_sealed(oracle, n, adlen)
    dec = aead.new_decryptor(KEY)
    assert dec.decrypt(NONCE, out, ad) == pt
    bad = bytearray(out)
    bad[n // 2] ^= 4
    with pytest.raises(TlsError) as e:
        dec.decrypt(NONCE, bytes(bad), ad)
    assert e.value.kind is TlsErrorKind.BadRecordMac and e.value.desc == "wrong mac"


@pytest.mark.parametrize("g", [1, 2, 3, 0])
def test_tile_edges_device_form(gpu, oracle, key_t, groups, g):
    T = tile_bytes()
    groups(g)
    for adlen in (0, 5, 13, 24):
        for total in (T - 1, T, T + 1, 2 * T - 9, 2 * T - 4, 2 * T, 3 * T + 5):
            n = total - adlen - 16
            pt, ad = data(n), data(adlen, 2)
            want = want_sealed(oracle, n, adlen)
            assert seal_dev(key_t, pt, ad) == want, (g, adlen, total)
            assert open_dev(key_t, want, ad) == (SG_OK, SG_OK, pt), (g, adlen, total)


def test_many_tiles_per_group_on_the_automatic_grid(gpu, oracle, key_t, groups):
    from suruga_amd import msg

    groups(0)
    n = (8 << 20) + 1000
    assert msg.plan_for(n, 13)["tiles_per_group"] >= 1 and msg.plan_for(n, 13)["groups"] > 256
    pt, ad = data(n), data(13, 2)
    want = want_sealed(oracle, n, 13)
    assert seal_dev(key_t, pt, ad) == want
    assert open_dev(key_t, want, ad) == (SG_OK, SG_OK, pt)
    groups(5)  # ... and really many: 103 tiles per group
    assert msg.plan_for(n, 13, 5)["tiles_per_group"] > 100
    assert seal_dev(key_t, pt, ad) == want


@pytest.mark.parametrize("off_in", [0, 1, 3])
@pytest.mark.parametrize("off_out", [0, 1, 3])
def test_alignment(gpu, oracle, key_t, off_in, off_out):
    n = 2 * tile_bytes() + 33
    pt = data(n)
    for off_ad in (0, 1, 3):
        ad = data(13, 2)
        want = want_sealed(oracle, n, 13)
        offs = (off_in, off_out, off_ad)
        assert seal_dev(key_t, pt, ad, offs) == want, offs
        assert open_dev(key_t, want, ad, offs) == (SG_OK, SG_OK, pt), offs


def test_in_place(gpu, oracle, key_t):
    import torch

    from suruga_amd import msg

    n = 3 * tile_bytes() + 5
    pt, ad = data(n), data(13, 2)
    want = want_sealed(oracle, n, 13)
    for off in (0, 3):
        buf, adt = dev(pt, off, room=16), dev(ad)
        msg.seal_msg(key_t, NONCE, buf, buf, ad=adt, in_len=n, stream=0)
        assert host(buf) == want
        st = torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")
        assert msg.open_(key_t, NONCE, buf, buf, st, ad=adt, in_len=n + 16, stream=0) == SG_OK
        assert int(st.item()) == SG_OK
        assert host(buf) == pt + want[n:]  # the tag behind the plaintext is left alone


def test_tamper(gpu, oracle, key_t):
    from suruga_amd import ChaCha20Poly1305

    T = tile_bytes()
    n = 3 * T + 5
    pt, ad = data(n), data(13, 2)
    sealed = want_sealed(oracle, n, 13)
    dec = ChaCha20Poly1305().new_decryptor(KEY)
    for where in ("first", "middle tile", "last", "tag", "ad"):
        ct, bad_ad = bytearray(sealed), bytearray(ad)
        if where == "ad":
            bad_ad[6] ^= 0x10
        else:
            ct[{"first": 0, "middle tile": T + T // 2, "last": n - 1, "tag": n + 9}[where]] ^= 0x01
        ct, bad_ad = bytes(ct), bytes(bad_ad)
        rc_o, plain_o = oracle.open(KEY, NONCE, ct, bad_ad)
        assert rc_o == SG_E_BAD_MAC
        # default: the output of a failed open is zeroed on the device
        assert open_dev(key_t, ct, bad_ad) == (SG_OK, SG_E_BAD_MAC, bytes(n)), where
        assert open_dev(key_t, ct, bad_ad, offs=(0, 3, 0)) == (SG_OK, SG_E_BAD_MAC, bytes(n)), where
        # SG_MSG_KEEP_FAILED: the unauthenticated plaintext, which the decryption always produces
        assert open_dev(key_t, ct, bad_ad, keep_failed=True) == (SG_OK, SG_E_BAD_MAC, plain_o), where
        # host form: SG_E_BAD_MAC and a zeroed out
        back = (C.c_uint8 * n)(*([0xEE] * 64))
        assert gpu.sg_open_msg(dec._ptr, NONCE, 8, ct, n + 16, bad_ad, len(bad_ad), back) == SG_E_BAD_MAC, where
        assert bytes(back) == bytes(n), where
    # fewer bytes than a tag: SG_E_SHORT, nothing touched
    rc, st, _ = open_dev(key_t, bytes(16), b"")
    assert rc == SG_OK
    import torch

    from suruga_amd import msg

    stt = torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")
    out = dev(b"", room=16)
    assert msg.open_(key_t, NONCE, dev(bytes(15)), out, stt, in_len=15, stream=0) == SG_E_SHORT
    assert int(stt.item()) == 0xFF
    back = (C.c_uint8 * 16)()
    assert gpu.sg_open_msg(dec._ptr, NONCE, 8, bytes(15), 15, b"", 0, back) == SG_E_SHORT


def test_asynchronous_on_a_stream(gpu, oracle, key_t):
    """A call on a non-NULL stream returns while a large fill enqueued before it
    on that stream is still running; the result is right once the stream is done."""
    import torch

    from suruga_amd import msg

    n = 3 * tile_bytes() + 5
    pt, ad = data(n), data(13, 2)
    inp, adt, out = dev(pt), dev(ad), dev(b"", room=n + 16)
    ws = torch.empty(msg.workspace_size(), dtype=torch.uint8, device="cuda")
    s = torch.cuda.Stream()
    msg.seal_msg(key_t, NONCE, inp, out, ad=adt, in_len=n, stream=s, workspace=ws)  # warm: code objects loaded
    s.synchronize()
    out.zero_()
    big = torch.empty(1 << 30, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    filled = torch.cuda.Event()
    with torch.cuda.stream(s):
        for _ in range(16):  # 16 GiB of stores: milliseconds
            big.fill_(7)
        filled.record(s)
    msg.seal_msg(key_t, NONCE, inp, out, ad=adt, in_len=n, stream=s, workspace=ws)
    returned_early = not filled.query()
    s.synchronize()
    assert returned_early, "sg_seal_msg_dev waited for the stream's earlier work"
    assert host(out) == want_sealed(oracle, n, 13)


def test_cpp_trait_dispatch(gpu):
    """include/suruga/cipher.hpp: 40,000 bytes with 300 bytes of AD through the
    C++ Encryptor / Decryptor, in a child process (tests/cpp/test_msg.cpp)."""
    from suruga_amd import _build

    binary = _build.build_cpp_msg_test()
    proc = subprocess.run([str(binary)], capture_output=True, text=True, timeout=120)
    assert proc.returncode == 0, proc.stdout + proc.stderr
    assert "0 failed" in proc.stdout
