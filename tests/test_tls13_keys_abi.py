"""sg_tls13_traffic_keys_dev and the context's traffic-secret calls reject bad
arguments before any GPU work, so the checks are pinned here on the CPU with dummy
device addresses (never dereferenced), as tests/test_abi.py does; and the ctypes
mirror of sg_tls13_keys has the header's layout.  CPU only."""
from __future__ import annotations

import ctypes as C
import re

import pytest

from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def good():
    from suruga_amd._native import SgTls13Keys

    k = SgTls13Keys()
    k.count, k.rows, k.flags = 4, 4, 0
    k.secrets, k.keys, k.ivs = 0x1000, 0x2000, 0x3000
    return k


def test_struct_layout_matches_the_header():
    from suruga_amd._native import SG_TLS13_KEYS_UPDATE, SgTls13Keys

    text = (ROOT / "include" / "suruga_gpu.h").read_text()
    body = re.search(r"typedef struct sg_tls13_keys \{(.*?)\} sg_tls13_keys;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*;", body)
    assert names == [n for n, _ in SgTls13Keys._fields_] == ["count", "flags", "rows", "_pad", "index", "secrets",
                                                             "keys", "ivs", "stream"]
    assert C.sizeof(SgTls13Keys) == 56
    offsets = {n: getattr(SgTls13Keys, n).offset for n in names}
    assert offsets == {"count": 0, "flags": 4, "rows": 8, "_pad": 12, "index": 16, "secrets": 24, "keys": 32, "ivs": 40,
                       "stream": 48}
    assert re.search(r"#define\s+SG_TLS13_KEYS_UPDATE\s+0x1u", text) and SG_TLS13_KEYS_UPDATE == 1


def test_argument_errors_before_any_gpu_call(lib):
    from suruga_amd._native import SG_E_ARG, SG_TLS13_KEYS_UPDATE

    def rejected(what, **fields):
        k = good()
        for name, v in fields.items():
            setattr(k, name, v)
        assert lib.sg_tls13_traffic_keys_dev(C.byref(k)) == SG_E_ARG, what
        assert lib.sg_last_error(), what

    assert lib.sg_tls13_traffic_keys_dev(None) == SG_E_ARG
    rejected("unknown flags", flags=0x2)
    rejected("unknown flags beside UPDATE", flags=SG_TLS13_KEYS_UPDATE | 0x80000000)
    rejected("NULL secrets", secrets=None)
    for field in ("secrets", "keys", "ivs", "index"):
        for off in (1, 2, 3):
            rejected(f"misaligned {field}", **{field: 0x4000 + off})
    rejected("no table and no update", keys=None, ivs=None)
    rejected("count above rows without an index", count=5)
    # every one of them also with count == 0: the arguments are checked first
    rejected("unknown flags, empty", flags=0x4, count=0)
    rejected("NULL secrets, empty", secrets=None, count=0)


def test_empty_call_launches_nothing(lib):
    from suruga_amd._native import SG_TLS13_KEYS_UPDATE

    k = good()
    k.count = 0
    assert lib.sg_tls13_traffic_keys_dev(C.byref(k)) == 0
    k.flags, k.keys, k.ivs = SG_TLS13_KEYS_UPDATE, None, None  # an update alone is a call
    assert lib.sg_tls13_traffic_keys_dev(C.byref(k)) == 0
    k.rows, k.index = 0, 0x5000  # rows bounds the index entries, not count
    assert lib.sg_tls13_traffic_keys_dev(C.byref(k)) == 0


def test_context_calls_reject_null(lib):
    from suruga_amd._native import SG_E_ARG

    assert lib.sg_ctx_key_update(None) == SG_E_ARG
    assert lib.sg_ctx_set_traffic_secret(None, bytes(32)) == SG_E_ARG
    dummy = C.create_string_buffer(64)  # never dereferenced: the NULL secret is refused first
    assert lib.sg_ctx_set_traffic_secret(C.cast(dummy, C.c_void_p), None) == SG_E_ARG


def test_kernel_file_is_part_of_the_build_and_the_source_hash():
    from suruga_amd import _build

    names = [p.name for p in _build.HIP_SOURCES]
    assert "sg_hkdf.hip" in names
    deps = [p.name for p in _build.HIP_DEPS]
    assert "sg_hkdf.hip" in deps and "sg_hkdf.h" in deps
