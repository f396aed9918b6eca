"""sg_derive_keys_ivs (sg_keysched.cpp): the 88-byte key block of RFC 5246
section 6.3 with no MAC keys -- two 32-byte keys, then the two 12-byte write IVs
of RFC 7905 section 2 -- against the oracle's PRF restatement (oracle/tls_prf.py),
and its first 64 bytes against sg_derive_keys.  CPU only."""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import tls_prf as ORC  # noqa: E402  (test infrastructure)

from suruga_amd import keysched as K  # noqa: E402

COUNT = 16


def inputs():
    rng = np.random.default_rng(7905)
    return (rng.integers(0, 256, (COUNT, 48), dtype=np.uint8), rng.integers(0, 256, (COUNT, 32), dtype=np.uint8),
            rng.integers(0, 256, (COUNT, 32), dtype=np.uint8))


def key_block(pm: bytes, cr: bytes, sr: bytes):
    master = ORC.Prf(pm, b"master secret" + cr + sr).get_bytes(48)
    return master, ORC.Prf(master, b"key expansion" + sr + cr).get_bytes(88)


@pytest.mark.parametrize("threads", [1, 4])
def test_all_88_bytes_against_the_oracle_prf(threads):
    pm, cr, sr = inputs()
    cw, sw, ci, si, ms = K.derive_keys_ivs(pm, cr, sr, threads=threads, with_master=True)
    assert ci.shape == si.shape == (COUNT, 12)
    for i in range(COUNT):
        master, kb = key_block(pm[i].tobytes(), cr[i].tobytes(), sr[i].tobytes())
        got = cw[i].tobytes() + sw[i].tobytes() + ci[i].tobytes() + si[i].tobytes()
        assert got == kb, i
        assert ms[i].tobytes() == master, i
        assert ORC.derive_keys(pm[i].tobytes(), cr[i].tobytes(), sr[i].tobytes()) == (master, kb[:32], kb[32:64])


@pytest.mark.parametrize("threads", [1, 4])
def test_first_64_bytes_are_sg_derive_keys(threads):
    pm, cr, sr = inputs()
    cw, sw, ci, si = K.derive_keys_ivs(pm, cr, sr, threads=threads)
    cw0, sw0 = K.derive_keys(pm, cr, sr, threads=threads)
    assert np.array_equal(cw, cw0) and np.array_equal(sw, sw0)
    assert len({ci[i].tobytes() for i in range(COUNT)} | {si[i].tobytes() for i in range(COUNT)}) == 2 * COUNT


def test_null_iv_outputs_are_rejected():
    import ctypes as C

    from suruga_amd import _native as N

    pm, cr, sr = inputs()
    cw = np.empty((COUNT, 32), dtype=np.uint8)
    sw = np.empty((COUNT, 32), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = N.load().sg_derive_keys_ivs(COUNT, p(pm), 48, 48, p(cr), p(sr), None, p(cw), p(sw), None, None, 1)
    assert rc == N.SG_E_ARG
