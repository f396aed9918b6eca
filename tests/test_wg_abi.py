"""sg_seal_batch_wg / sg_open_batch_wg reject bad arguments before any GPU work, so the
checks are pinned here on the CPU with dummy device addresses (never dereferenced), as
tests/test_quic_abi.py does; the ctypes mirror of sg_wg_batch has the header's layout; and
the host-only helpers sg_wg_padded_len and sg_wg_message_len say what tests/wg_ref.py says.
CPU only."""
from __future__ import annotations

import ctypes as C
import re

import pytest

import wg_ref as W
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def good():
    from suruga_amd._native import SgWgBatch

    b = SgWgBatch()
    b.count, b.flags, b.num_keys, b.pad_cap = 4, 0, 2, 1420
    b.keys, b.receiver, b.status = 0x1000, 0x2000, 0x6000
    b.counter, b.counter_out = 0x4000, 0x5000
    b.in_, b.out = 0x10001, 0x20003  # packets lie at any address
    b.uniform_len, b.in_stride, b.out_stride = 1200, 1216, 1248
    return b


FIELDS = ["count", "flags", "keys", "receiver", "key_index", "counter", "counter_out", "inner_len", "num_keys", "pad_cap",
          "in", "in_off", "in_stride", "out", "out_off", "out_stride", "len", "uniform_len", "max_len", "status", "stream"]


def test_struct_layout_matches_the_header():
    from suruga_amd import _native as N

    text = (ROOT / "include" / "suruga_gpu.h").read_text()
    body = re.search(r"typedef struct sg_wg_batch \{(.*?)\} sg_wg_batch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == FIELDS
    assert [n.rstrip("_") for n, _ in N.SgWgBatch._fields_] == FIELDS
    assert C.sizeof(N.SgWgBatch) == 144 and "144 bytes" in text
    host = (ROOT / "suruga_amd" / "csrc" / "sg_wg_host.cpp").read_text()
    assert "static_assert(sizeof(sg_wg_batch) == 144" in host
    off = {n.rstrip("_"): getattr(N.SgWgBatch, n).offset for n, _ in N.SgWgBatch._fields_}
    assert off == {"count": 0, "flags": 4, "keys": 8, "receiver": 16, "key_index": 24, "counter": 32, "counter_out": 40,
                   "inner_len": 48, "num_keys": 56, "pad_cap": 60, "in": 64, "in_off": 72, "in_stride": 80, "out": 88,
                   "out_off": 96, "out_stride": 104, "len": 112, "uniform_len": 120, "max_len": 124, "status": 128,
                   "stream": 136}
    for name, v in (("SG_WG_HEADER_LEN", 16), ("SG_WG_MAX_MESSAGE_LEN", 16384), ("SG_WG_KEEP_FAILED", 1),
                    ("SG_STATUS_BAD_HEADER", 6), ("SG_STATUS_BAD_INNER", 7)):
        m = re.search(r"#define\s+%s\s+(\w+?)u?\s" % name, text)
        assert m and int(m.group(1), 0) == v == getattr(N, name), name
    assert (W.BAD_HEADER, W.BAD_INNER, W.HEADER_LEN, W.MAX_MESSAGE_LEN) == (6, 7, 16, 16384)
    for sym in ("sg_seal_batch_wg", "sg_open_batch_wg", "sg_wg_padded_len", "sg_wg_message_len"):
        assert sym in N.EXPORTS and re.search(r"\b%s\(" % sym, text)
    # the wire format, stated in the header comment exactly
    for line in ("le32(4)                       type 4, three reserved zero bytes",
                 "le32(receiver)                the peer's index for this session",
                 "le64(counter)",
                 "AEAD(key, nonce = 00 00 00 00 || le64(counter), plaintext = inner || zeros, AD = empty)   -> P bytes || 16-byte tag"):
        assert line in text, line


@pytest.mark.parametrize("open_", (False, True))
def test_argument_errors_before_any_gpu_call(lib, open_):
    from suruga_amd._native import SG_E_ARG, SG_WG_KEEP_FAILED

    call = lib.sg_open_batch_wg if open_ else lib.sg_seal_batch_wg

    def rejected(what, **fields):
        for count in (4, 0):  # the arguments are checked first, also of an empty call
            b = good()
            b.count = count
            for name, v in fields.items():
                setattr(b, name, v)
            assert call(C.byref(b)) == SG_E_ARG, (what, count)
            assert lib.sg_last_error(), what

    assert call(None) == SG_E_ARG and lib.sg_last_error()
    rejected("unknown flags", flags=0x2)
    rejected("unknown flags beside the known", flags=SG_WG_KEEP_FAILED | 0x80000000)
    for field in ("keys", "status", "in_", "out"):
        rejected(f"NULL {field}", **{field: None})
    if open_:
        rejected("open without counter_out", counter_out=None)
    else:
        rejected("seal without receiver", receiver=None)
        rejected("seal without counter", counter=None)
    for field in ("receiver", "key_index", "inner_len", "len"):
        for o in (1, 2, 3):
            rejected(f"misaligned {field}", **{field: 0x7000 + o}, max_len=1200)
    for field in ("counter", "counter_out", "in_off", "out_off"):
        for o in (1, 2, 4, 7):
            rejected(f"misaligned {field}", **{field: 0x8000 + o})
    rejected("num_keys 0", num_keys=0)
    rejected("pad_cap above the inner bound", pad_cap=16384 - 32 + 1)
    rejected("pad_cap far above", pad_cap=0xFFFFFFFF)
    limit = 16384 if open_ else 16384 - 32
    rejected("uniform_len above the bound", uniform_len=limit + 1)
    rejected("max_len above the bound", len=0x9000, max_len=limit + 1)
    rejected("max_len far above", len=0x9000, max_len=0xFFFFFFFF)


@pytest.mark.parametrize("open_", (False, True))
def test_empty_call_launches_nothing(lib, open_):
    from suruga_amd._native import SG_WG_KEEP_FAILED

    call = lib.sg_open_batch_wg if open_ else lib.sg_seal_batch_wg
    limit = 16384 if open_ else 16384 - 32
    b = good()
    b.count = 0
    assert call(C.byref(b)) == 0
    b.flags, b.uniform_len, b.pad_cap = SG_WG_KEEP_FAILED, limit, 16384 - 32
    assert call(C.byref(b)) == 0
    b.len, b.max_len, b.uniform_len = 0xA000, limit, 0xFFFFFFFF  # with a length array uniform_len is not read
    assert call(C.byref(b)) == 0
    b.inner_len, b.key_index, b.in_off, b.out_off = 0xB000, 0xB100, 0xB200, 0xB300
    assert call(C.byref(b)) == 0
    if open_:
        b.receiver, b.counter = None, None  # open reads neither
    else:
        b.counter_out = None                # seal does not read it
    assert call(C.byref(b)) == 0


def test_length_functions_against_the_reference(lib):
    for cap in (0, 1420, 1500):
        for n in range(0, 131):
            assert lib.sg_wg_padded_len(n, cap) == W.padded_len(n, cap), (n, cap)
            assert lib.sg_wg_message_len(n, cap) == W.message_len(n, cap) == 32 + W.padded_len(n, cap), (n, cap)
        for n in range(1400, 1520):  # across both caps
            assert lib.sg_wg_padded_len(n, cap) == W.padded_len(n, cap), (n, cap)
            assert lib.sg_wg_message_len(n, cap) == W.message_len(n, cap), (n, cap)
    # ragged caps, and the ends of 32 bits: nothing wraps
    for cap in (1, 15, 17, 100):
        for n in range(0, 131):
            assert lib.sg_wg_padded_len(n, cap) == W.padded_len(n, cap), (n, cap)
    assert lib.sg_wg_padded_len(0xFFFFFFF0, 0) == 0xFFFFFFF0 and lib.sg_wg_padded_len(0xFFFFFFF1, 0) == 0xFFFFFFF1
    assert lib.sg_wg_padded_len(0xFFFFFFFF, 0xFFFFFFFF) == 0xFFFFFFFF
    assert lib.sg_wg_message_len(0xFFFFFFDF, 0) == 0xFFFFFFFF and lib.sg_wg_message_len(0xFFFFFFC0, 0) == 0xFFFFFFE0


def test_python_surface(lib):
    import suruga_amd
    from suruga_amd import wg

    assert {"WgBatch", "seal_wg", "open_wg", "padded_len", "message_len", "SG_STATUS_BAD_HEADER",
            "SG_STATUS_BAD_INNER"} <= set(suruga_amd.__all__)
    assert (suruga_amd.SG_STATUS_BAD_HEADER, suruga_amd.SG_STATUS_BAD_INNER) == (6, 7)
    assert wg.padded_len(1419, 1420) == 1420 and wg.message_len(17) == 64 and suruga_amd.padded_len(0) == 0


def test_kernel_file_is_part_of_the_build_and_the_source_hash():
    from suruga_amd import _build

    names = [p.name for p in _build.HIP_SOURCES]
    assert {"sg_wg.hip", "sg_wg_capi.cpp", "sg_wg_host.cpp"} <= set(names)
    assert "sg_wg.h" in [p.name for p in _build.HIP_DEPS]
    # the host-only files stay free of HIP
    for f in ("sg_wg.h", "sg_wg_host.cpp"):
        text = (_build.CSRC / f).read_text()
        assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text, f
    census = (ROOT / "tools" / "isa_census.py").read_text()
    assert '"sg_wg.hip"' in census
