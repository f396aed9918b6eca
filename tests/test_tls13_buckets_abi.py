"""CPU tests of sg_set_tls13_buckets (include/suruga_gpu.h): the symbol, its query / set /
restore contract, its initial value -- 0, or what SG_TLS13_BUCKETS says, read in a fresh
process -- and that the header and the Python binding declare it.  No GPU call is made."""
from __future__ import annotations

import os
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def test_symbol_and_contract(lib):
    """Returns the previous setting; a negative argument only queries."""
    fn = lib.sg_set_tls13_buckets
    start = fn(-1)
    assert start in (0, 1) and fn(-1) == start and fn(-7) == start
    try:
        assert fn(1) == start and fn(-1) == 1
        assert fn(0) == 1 and fn(-1) == 0
        assert fn(5) == 0 and fn(-1) == 1  # any positive value is "on"
    finally:
        fn(start)
    assert fn(-1) == start


def test_python_mirror(lib):
    from suruga_amd import batch as B

    start = B.set_tls13_buckets(-1)
    try:
        assert B.set_tls13_buckets(1) == start and lib.sg_set_tls13_buckets(-1) == 1
        assert B.set_tls13_buckets(0) == 1 and B.set_tls13_buckets(-1) == 0
    finally:
        B.set_tls13_buckets(start)


def child(env_value):
    """(initial value, value after flipping it) in a fresh process."""
    env = {k: v for k, v in os.environ.items() if k != "SG_TLS13_BUCKETS"}
    if env_value is not None:
        env["SG_TLS13_BUCKETS"] = env_value
    code = ("from suruga_amd import _native as N; lib = N.load(); a = lib.sg_set_tls13_buckets(-1); "
            "lib.sg_set_tls13_buckets(1 - a); print(a, lib.sg_set_tls13_buckets(-1))")
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return tuple(int(x) for x in p.stdout.split())


@pytest.mark.parametrize("env_value, initial", [(None, 0), ("1", 1), ("0", 0)])
def test_initial_value_in_a_fresh_process(lib, env_value, initial):
    """Off unless the environment asks for it; the setter then overrides the environment."""
    assert child(env_value) == (initial, 1 - initial)


def test_the_other_switches_keep_their_defaults(lib):
    code = ("from suruga_amd import _native as N; lib = N.load(); "
            "print(lib.sg_set_lockstep(-1), lib.sg_set_packed(-1), lib.sg_set_tls13_buckets(-1))")
    env = {k: v for k, v in os.environ.items() if k not in ("SG_TLS13_BUCKETS", "SG_LOCKSTEP", "SG_PACK")}
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.split() == ["1", "1", "0"], p.stdout + p.stderr


def test_header_and_binding_declare_it():
    from suruga_amd._native import EXPORTS

    text = (ROOT / "include" / "suruga_gpu.h").read_text()
    assert re.search(r"^int sg_set_tls13_buckets\(int enable\);", text, re.M)
    assert "SG_TLS13_BUCKETS" in text
    assert "sg_set_tls13_buckets" in EXPORTS


def test_the_batch_structs_carry_no_such_option(lib):
    """The switch is process state: sg_batch_tls13.flags and sg_tls13_seal_opts.flags stay
    must-be-zero fields (tests/test_tls13_batch_abi.py and test_tls13_pad_abi.py hold the values)."""
    import ctypes as C

    from suruga_amd._native import SG_BATCH_TLS, SG_E_ARG, SgBatch, SgBatchTls13, SgTls13SealOpts

    b = SgBatch()
    b.count, b.num_keys, b.flags = 4, 1, SG_BATCH_TLS
    b.keys, b.in_, b.out = 0x1000, 0x20000, 0x300000
    b.content_type = 23
    b.uniform_len, b.in_stride, b.out_stride = 64, 64, 160
    prev = lib.sg_set_tls13_buckets(1)
    try:
        for flags in (1, 0x100, 0x80000000):
            x, o = SgBatchTls13(), SgTls13SealOpts()
            x.ivs, x.flags = 0x5000, flags
            assert lib.sg_seal_batch_tls13(C.byref(b), C.byref(x)) == SG_E_ARG
            x.flags, o.pad_to, o.flags = 0, 64, flags
            assert lib.sg_seal_batch_tls13_ex(C.byref(b), C.byref(x), C.byref(o)) == SG_E_ARG
    finally:
        lib.sg_set_tls13_buckets(prev)
