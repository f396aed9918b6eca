"""sg_seal_batch_dtls13 / sg_open_batch_dtls13 reject bad arguments before any GPU work, so
the checks are pinned here on the CPU with dummy device addresses (never dereferenced), as
tests/test_esp_abi.py does; the ctypes mirror of sg_dtls13_batch has the header's layout;
the host-only helpers sg_dtls13_header_len, sg_dtls13_inner_len and sg_dtls13_record_len say
what tests/dtls13_ref.py says; and sg_dtls13_record_keys gives the fixture's keys.  CPU only."""
from __future__ import annotations

import ctypes as C
import re

import numpy as np
import pytest

import dtls13_ref as D
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def good(open_: bool):
    from suruga_amd._native import SgDtls13Batch

    b = SgDtls13Batch()
    b.count, b.flags, b.num_conns, b.cid_len, b.uniform_type = 4, 0, 2, 8, 23
    b.keys, b.ivs, b.sn_keys, b.cids, b.status = 0x1000, 0x2000, 0x3000, 0x3801, 0x6000
    if open_:
        b.expected, b.seq_out, b.epoch_out, b.content_len, b.type_out = 0x4000, 0x5000, 0x5801, 0x5C00, 0x5E03
    else:
        b.seq = 0x4000
    b.in_, b.out = 0x10001, 0x20003  # records lie at any address
    b.uniform_len, b.in_stride, b.out_stride = 1200, 1216, 1248
    return b


FIELDS = ["count", "flags", "keys", "ivs", "sn_keys", "cids", "key_index", "seq", "type", "epoch", "expected", "seq_out",
          "epoch_out", "content_len", "type_out", "num_conns", "cid_len", "pad_to", "uniform_type", "uniform_epoch", "in",
          "in_off", "in_stride", "out", "out_off", "out_stride", "len", "uniform_len", "max_len", "status", "stream"]


def test_struct_layout_matches_the_header():
    from suruga_amd import _native as N

    text = (ROOT / "include" / "suruga_gpu.h").read_text()
    body = re.search(r"typedef struct sg_dtls13_batch \{(.*?)\} sg_dtls13_batch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == FIELDS
    assert [n.rstrip("_") if n == "in_" else n for n, _ in N.SgDtls13Batch._fields_] == FIELDS
    assert C.sizeof(N.SgDtls13Batch) == 208 and "208 bytes" in text
    host = (ROOT / "suruga_amd" / "csrc" / "sg_dtls13_host.cpp").read_text()
    assert "static_assert(sizeof(sg_dtls13_batch) == 208" in host
    off = {(n.rstrip("_") if n == "in_" else n): getattr(N.SgDtls13Batch, n).offset for n, _ in N.SgDtls13Batch._fields_}
    assert off == {"count": 0, "flags": 4, "keys": 8, "ivs": 16, "sn_keys": 24, "cids": 32, "key_index": 40, "seq": 48,
                   "type": 56, "epoch": 64, "expected": 72, "seq_out": 80, "epoch_out": 88, "content_len": 96, "type_out": 104,
                   "num_conns": 112, "cid_len": 116, "pad_to": 120, "uniform_type": 124, "uniform_epoch": 125, "in": 128,
                   "in_off": 136, "in_stride": 144, "out": 152, "out_off": 160, "out_stride": 168, "len": 176,
                   "uniform_len": 184, "max_len": 188, "status": 192, "stream": 200}
    for name, v in (("SG_DTLS13_MAX_CONTENT_LEN", 16384), ("SG_DTLS13_MAX_CID_LEN", 250), ("SG_DTLS13_SEQ16", 1),
                    ("SG_DTLS13_LENGTH", 2), ("SG_DTLS13_EPOCH_ROWS", 4), ("SG_DTLS13_KEEP_FAILED", 8), ("SG_STATUS_BAD_HEADER", 6)):
        m = re.search(r"#define\s+%s\s+(\w+?)u?\s" % name, text)
        assert m and int(m.group(1), 0) == v == getattr(N, name), name
    assert re.search(r"#define\s+SG_DTLS13_MAX_RECORD_LEN\s+\(255u \+ 16384u \+ 1u \+ 16u\)", text)
    assert N.SG_DTLS13_MAX_RECORD_LEN == D.MAX_RECORD_LEN == 255 + 16384 + 1 + 16
    assert re.search(r"#define\s+SG_STATUS_NO_TYPE\s+5\s", text)
    assert (D.NO_TYPE, D.BAD_HEADER, D.MAX_CONTENT_LEN, D.MAX_CID_LEN, D.MAX_INNER) == (5, 6, 16384, 250, 16385)
    for sym in ("sg_seal_batch_dtls13", "sg_open_batch_dtls13", "sg_dtls13_header_len", "sg_dtls13_inner_len",
                "sg_dtls13_record_len", "sg_dtls13_record_keys"):
        assert sym in N.EXPORTS and re.search(r"\b%s\(" % sym, text)
    # the wire format, stated in the header comment exactly
    for line in ("0 0 1 C S L E E                     first byte: C = 0x10, S = 0x08, L = 0x04, EE = epoch mod 4",
                 "connection ID, cid_len bytes        where C is set",
                 "sequence number, low 8 bits (S = 0) or low 16 bits (S = 1), big-endian",
                 "be16(|encrypted_record|)            where L is set",
                 "encrypted_record = AEAD(key, nonce = iv XOR (00 00 00 00 || be64(seq)),",
                 "     plaintext = content || u8(type) || zeros,"):
        assert " *   " + line + "\n" in text, line


@pytest.mark.parametrize("open_", (False, True))
def test_argument_errors_before_any_gpu_call(lib, open_):
    from suruga_amd._native import SG_DTLS13_KEEP_FAILED, SG_E_ARG

    call = lib.sg_open_batch_dtls13 if open_ else lib.sg_seal_batch_dtls13

    def rejected(what, **fields):
        for count in (4, 0):  # the arguments are checked first, also of an empty call
            b = good(open_)
            b.count = count
            for name, v in fields.items():
                setattr(b, name, v)
            assert call(C.byref(b)) == SG_E_ARG, (what, count)
            assert lib.sg_last_error(), what

    assert call(None) == SG_E_ARG and lib.sg_last_error()
    rejected("unknown flags", flags=0x10)
    rejected("unknown flags beside the known", flags=SG_DTLS13_KEEP_FAILED | 0x80000000)
    for field in ("keys", "ivs", "sn_keys", "status", "in_", "out"):
        rejected(f"NULL {field}", **{field: None})
    if open_:
        for field in ("expected", "seq_out", "epoch_out", "content_len", "type_out"):
            rejected(f"open without {field}", **{field: None})
        for o in (1, 2, 3):
            rejected("misaligned content_len", content_len=0x7000 + o)
    else:
        rejected("seal without seq", seq=None)
        rejected("seal with a cid_len and no cids", cids=None)
        rejected("... at the longest", cids=None, cid_len=250)
    for field in ("ivs", "key_index", "len"):
        for o in (1, 2, 3):
            rejected(f"misaligned {field}", **{field: 0x7000 + o}, max_len=1200)
    for field in ("seq", "expected", "seq_out", "in_off", "out_off"):
        for o in (1, 2, 4, 7):
            rejected(f"misaligned {field}", **{field: 0x8000 + o})
    rejected("num_conns 0", num_conns=0)
    for c in (251, 255, 256, 0xFFFFFFFF):
        rejected(f"cid_len {c}", cid_len=c)
    for p in (2**14 + 1, 2**15, 0xFFFFFFFF):
        rejected(f"pad_to {p}", pad_to=p)
    # the bound: open on the record, seal on the content
    limit = D.MAX_RECORD_LEN if open_ else D.MAX_CONTENT_LEN
    rejected("uniform_len above the bound", uniform_len=limit + 1)
    rejected("max_len above the bound", len=0x9000, max_len=limit + 1)
    rejected("max_len far above", len=0x9000, max_len=0xFFFFFFFF)


@pytest.mark.parametrize("open_", (False, True))
def test_empty_call_launches_nothing(lib, open_):
    from suruga_amd import _native as N

    call = lib.sg_open_batch_dtls13 if open_ else lib.sg_seal_batch_dtls13
    limit = D.MAX_RECORD_LEN if open_ else D.MAX_CONTENT_LEN
    b = good(open_)
    b.count = 0
    assert call(C.byref(b)) == 0
    b.flags = N.SG_DTLS13_SEQ16 | N.SG_DTLS13_LENGTH | N.SG_DTLS13_EPOCH_ROWS | N.SG_DTLS13_KEEP_FAILED
    b.uniform_len, b.cid_len, b.pad_to, b.uniform_epoch, b.uniform_type = limit, 250, 2**14, 255, 0
    assert call(C.byref(b)) == 0
    b.len, b.max_len, b.uniform_len = 0xA000, limit, 0xFFFFFFFF  # with a length array uniform_len is not read
    assert call(C.byref(b)) == 0
    b.key_index, b.in_off, b.out_off, b.type, b.epoch = 0xB100, 0xB200, 0xB300, 0xB401, 0xB503
    assert call(C.byref(b)) == 0
    b.cid_len, b.cids = 0, None  # no connection ID: no table
    assert call(C.byref(b)) == 0
    if open_:
        b.seq, b.type, b.epoch, b.cids, b.cid_len = None, None, None, None, 9  # open reads none of them, cids included
    else:
        b.expected = b.seq_out = b.epoch_out = b.content_len = b.type_out = None  # seal reads none of them
        b.content_len = 0x7001                                                  # ... but the arrays' alignment holds for both
        assert call(C.byref(b)) == N.SG_E_ARG
        b.content_len = None
    assert call(C.byref(b)) == 0


def test_length_functions_against_the_reference(lib):
    from suruga_amd import _native as N

    for seq16 in (False, True):
        for length in (False, True):
            flags = (N.SG_DTLS13_SEQ16 if seq16 else 0) | (N.SG_DTLS13_LENGTH if length else 0)
            for cid_len in (0, 1, 11, 12, 250):
                hl = D.header_len(seq16, length, cid_len)
                assert lib.sg_dtls13_header_len(flags, cid_len) == hl
                assert lib.sg_dtls13_header_len(flags | N.SG_DTLS13_EPOCH_ROWS | N.SG_DTLS13_KEEP_FAILED, cid_len) == hl
                for n, pad_to in ((0, 0), (1431, 64), (16384, 256), (10000, 10000)):
                    assert lib.sg_dtls13_record_len(n, pad_to, flags, cid_len) == D.record_len(n, pad_to, seq16, length, cid_len)
    assert lib.sg_dtls13_header_len(0, 0) == 2 and lib.sg_dtls13_header_len(3, 11) == 16 and lib.sg_dtls13_header_len(3, 250) == 255
    for pad_to in (0, 1, 2, 16, 64, 100, 256, 4096, 10000, 2**14):
        for n in list(range(0, 601)) + list(range(16000, 16400)):
            assert lib.sg_dtls13_inner_len(n, pad_to) == D.inner_len(n, pad_to), (n, pad_to)
    # the cap: padding never carries the inner plaintext beyond 2^14 + 1, and a full content is not padded
    assert lib.sg_dtls13_inner_len(16383, 256) == 16384 and lib.sg_dtls13_inner_len(16384, 256) == 16385
    assert lib.sg_dtls13_inner_len(9999, 10000) == 10000 and lib.sg_dtls13_inner_len(10000, 10000) == 16385 and lib.sg_dtls13_inner_len(16384, 2**14) == 16385
    assert lib.sg_dtls13_inner_len(1, 2**14) == 2**14 and lib.sg_dtls13_inner_len(16385, 64) == 16386
    assert lib.sg_dtls13_record_len(16384, 0, 3, 250) == D.MAX_RECORD_LEN
    # the ends of 32 bits: nothing wraps
    assert lib.sg_dtls13_inner_len(0xFFFFFFFE, 64) == 0xFFFFFFFF and lib.sg_dtls13_inner_len(0xFFFFFFFF, 0) == 0xFFFFFFFF
    assert lib.sg_dtls13_record_len(0xFFFFFFEC, 0, 0, 0) == 0xFFFFFFFF and lib.sg_dtls13_record_len(0xFFFFFFEB, 0, 0, 0) == 0xFFFFFFFE
    assert lib.sg_dtls13_record_len(0xFFFFFFFF, 16, 3, 250) == 0xFFFFFFFF


def keys_call(lib, secrets, update, want=(True, True, True), threads=3):
    sec = np.array(secrets, dtype=np.uint8, order="C")
    n = sec.shape[0]
    out = [np.full((n, w), 0xEE, dtype=np.uint8) if on else None for w, on in zip((32, 12, 32), want)]
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    rc = lib.sg_dtls13_record_keys(n, p(sec), *(p(a) for a in out), int(update), threads)
    return rc, sec, out


def test_record_keys_against_the_fixture(lib):
    from suruga_amd._native import SG_E_ARG

    g = D.golden_keys()
    secrets = np.array([list(bytes.fromhex(c["secret"])) for c in g["cases"]], dtype=np.uint8)
    for threads in (1, 3, 64):
        rc, sec, (keys, ivs, sns) = keys_call(lib, secrets, False, threads=threads)
        assert rc == 0 and np.array_equal(sec, secrets)
        for i, c in enumerate(g["cases"]):
            assert (keys[i].tobytes().hex(), ivs[i].tobytes().hex(), sns[i].tobytes().hex()) == (c["key"], c["iv"], c["sn"]), i
    # with update: the next secret first, then its keys
    rc, sec, (keys, ivs, sns) = keys_call(lib, secrets, True)
    assert rc == 0
    for i, c in enumerate(g["cases"]):
        assert sec[i].tobytes().hex() == c["traffic upd"]
        assert (keys[i].tobytes(), ivs[i].tobytes(), sns[i].tobytes()) == D.record_keys(bytes.fromhex(c["traffic upd"]))
    chain = g["chain"]
    s = np.array([list(bytes.fromhex(chain[0]["secret"]))], dtype=np.uint8)
    for gen in chain[1:]:
        rc, s, (keys, ivs, sns) = keys_call(lib, s, True, threads=1)
        assert rc == 0 and s[0].tobytes().hex() == gen["secret"]
        assert (keys[0].tobytes().hex(), ivs[0].tobytes().hex(), sns[0].tobytes().hex()) == (gen["key"], gen["iv"], gen["sn"])
    # any table may be left out; nothing at all is an error, an empty call is not
    rc, _, (keys, ivs, sns) = keys_call(lib, secrets, False, want=(False, False, True))
    assert rc == 0 and sns[0].tobytes().hex() == g["cases"][0]["sn"]
    rc, sec, _ = keys_call(lib, secrets, True, want=(False, False, False))
    assert rc == 0 and sec[1].tobytes().hex() == g["cases"][1]["traffic upd"]
    assert keys_call(lib, secrets, False, want=(False, False, False))[0] == SG_E_ARG and lib.sg_last_error()
    assert lib.sg_dtls13_record_keys(3, None, None, None, None, 1, 1) == SG_E_ARG
    assert lib.sg_dtls13_record_keys(0, None, None, None, None, 0, 1) == 0
    # the TLS 1.3 labels are as they were: another prefix, other keys
    out = np.zeros(32, dtype=np.uint8)
    assert lib.sg_hkdf_expand_label(secrets[0].tobytes(), b"key", 3, None, 0, out.ctypes.data_as(C.c_void_p), 32) == 0
    assert out.tobytes().hex() != g["cases"][0]["key"]


def test_python_surface(lib):
    import suruga_amd
    from suruga_amd import dtls13

    assert {"Dtls13Batch", "seal_dtls13", "open_dtls13", "dtls13_header_len", "dtls13_inner_len", "dtls13_record_len",
            "dtls13_record_keys"} <= set(suruga_amd.__all__)
    assert dtls13.header_len() == 2 and dtls13.header_len(True, True, 8) == 13 and suruga_amd.dtls13_header_len(True, True, 250) == 255
    assert dtls13.inner_len(1200) == 1201 and dtls13.inner_len(1200, 64) == 1216 and suruga_amd.dtls13_inner_len(16384, 256) == 16385
    assert dtls13.record_len(1200, 0, True, True, 8) == 13 + 1201 + 16 == suruga_amd.dtls13_record_len(1200, 0, True, True, 8)
    g = D.golden_keys()
    sec = np.array([list(bytes.fromhex(c["secret"])) for c in g["cases"]], dtype=np.uint8)
    keys, ivs, sns = dtls13.record_keys(sec)
    assert keys[2].tobytes().hex() == g["cases"][2]["key"] and ivs.shape == (5, 12) and sns[4].tobytes().hex() == g["cases"][4]["sn"]
    keys, ivs, sns, nxt = suruga_amd.dtls13_record_keys(sec, update=True)
    assert nxt[0].tobytes().hex() == g["chain"][1]["secret"] and keys[0].tobytes().hex() == g["chain"][1]["key"]
    assert sec[0].tobytes().hex() == g["chain"][0]["secret"]  # the argument is left as it was
    with pytest.raises(ValueError):
        dtls13.record_keys(np.zeros((3, 31), dtype=np.uint8))
    with pytest.raises(ValueError):
        dtls13.seal_dtls13(dtls13.Dtls13Batch(count=0, keys=None, ivs=None, sn_keys=None, inp=None, out=None, status=None))
    with pytest.raises(ValueError):
        dtls13.open_dtls13(dtls13.Dtls13Batch(count=0, keys=None, ivs=None, sn_keys=None, inp=None, out=None, status=None))


def test_kernel_files_are_part_of_the_build_and_the_source_hash():
    from suruga_amd import _build

    names = [p.name for p in _build.HIP_SOURCES]
    assert {"sg_dtls13.hip", "sg_dtls13_capi.cpp", "sg_dtls13_host.cpp"} <= set(names)
    assert {"sg_dtls13.h", "sg_lane_aead.h"} <= {p.name for p in _build.HIP_DEPS}
    # the host-only files stay free of HIP
    for f in ("sg_dtls13.h", "sg_dtls13_host.cpp"):
        text = (_build.CSRC / f).read_text()
        assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text, f
    # the kernel is written on the shared steps, and the siblings are as they were
    kernel = (_build.CSRC / "sg_dtls13.hip").read_text()
    assert '#include "sg_lane_aead.h"' in kernel and "fmul_add" not in kernel
    for f in ("sg_quic.hip", "sg_wg.hip", "sg_esp.hip"):
        assert "sg_lane_aead.h" not in (_build.CSRC / f).read_text(), f
    census = (ROOT / "tools" / "isa_census.py").read_text()
    assert '"sg_dtls13.hip"' in census
