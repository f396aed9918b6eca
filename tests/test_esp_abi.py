"""sg_seal_batch_esp / sg_open_batch_esp reject bad arguments before any GPU work, so the
checks are pinned here on the CPU with dummy device addresses (never dereferenced), as
tests/test_wg_abi.py does; the ctypes mirror of sg_esp_batch has the header's layout; and
the host-only helpers sg_esp_padded_len, sg_esp_packet_len and sg_esp_seq_hi say what
tests/esp_ref.py says.  CPU only."""
from __future__ import annotations

import ctypes as C
import random
import re

import pytest

import esp_ref as E
from conftest import ROOT


@pytest.fixture(scope="module")
def lib():
    from suruga_amd import _build, _native

    _build.build_library()
    return _native.load()


def good():
    from suruga_amd._native import SgEspBatch

    b = SgEspBatch()
    b.count, b.flags, b.num_sas, b.align, b.uniform_next_header = 4, 0, 2, 4, 4
    b.keys, b.salts, b.spi, b.status = 0x1000, 0x2000, 0x3000, 0x6000
    b.seq, b.seq_out = 0x4000, 0x5000
    b.in_, b.out = 0x10001, 0x20003  # packets lie at any address
    b.uniform_len, b.in_stride, b.out_stride = 1200, 1216, 1248
    return b


FIELDS = ["count", "flags", "keys", "salts", "spi", "sa_index", "seq", "iv", "next_header", "seq_out", "payload_len",
          "next_header_out", "replay_top", "num_sas", "align", "uniform_next_header", "window", "in", "in_off", "in_stride",
          "out", "out_off", "out_stride", "len", "uniform_len", "max_len", "status", "stream"]


def test_struct_layout_matches_the_header():
    from suruga_amd import _native as N

    text = (ROOT / "include" / "suruga_gpu.h").read_text()
    body = re.search(r"typedef struct sg_esp_batch \{(.*?)\} sg_esp_batch;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == FIELDS
    assert [n.rstrip("_") if n == "in_" else n for n, _ in N.SgEspBatch._fields_] == FIELDS
    assert C.sizeof(N.SgEspBatch) == 192 and "192 bytes" in text
    host = (ROOT / "suruga_amd" / "csrc" / "sg_esp_host.cpp").read_text()
    assert "static_assert(sizeof(sg_esp_batch) == 192" in host
    off = {(n.rstrip("_") if n == "in_" else n): getattr(N.SgEspBatch, n).offset for n, _ in N.SgEspBatch._fields_}
    assert off == {"count": 0, "flags": 4, "keys": 8, "salts": 16, "spi": 24, "sa_index": 32, "seq": 40, "iv": 48,
                   "next_header": 56, "seq_out": 64, "payload_len": 72, "next_header_out": 80, "replay_top": 88,
                   "num_sas": 96, "align": 100, "uniform_next_header": 104, "window": 108, "in": 112, "in_off": 120,
                   "in_stride": 128, "out": 136, "out_off": 144, "out_stride": 152, "len": 160, "uniform_len": 168,
                   "max_len": 172, "status": 176, "stream": 184}
    for name, v in (("SG_ESP_HEADER_LEN", 16), ("SG_ESP_MAX_PACKET_LEN", 16384), ("SG_ESP_ESN", 1), ("SG_ESP_KEEP_FAILED", 2),
                    ("SG_STATUS_BAD_HEADER", 6), ("SG_STATUS_BAD_INNER", 7)):
        m = re.search(r"#define\s+%s\s+(\w+?)u?\s" % name, text)
        assert m and int(m.group(1), 0) == v == getattr(N, name), name
    assert (E.BAD_HEADER, E.BAD_INNER, E.HEADER_LEN, E.MAX_PACKET_LEN, E.MIN_PACKET) == (6, 7, 16, 16384, 34)
    for sym in ("sg_seal_batch_esp", "sg_open_batch_esp", "sg_esp_padded_len", "sg_esp_packet_len", "sg_esp_seq_hi"):
        assert sym in N.EXPORTS and re.search(r"\b%s\(" % sym, text)
    # the wire format, stated in the header comment exactly
    for line in ("be32(spi)",
                 "be32(seq_lo)                        low 32 bits of the sequence number",
                 "iv, 8 bytes                         be64(iv_i)",
                 "AEAD(key, nonce = salt(4) || iv(8),",
                 "     plaintext = payload || 01 02 .. pad || u8(pad) || u8(next_header),",
                 "     AD = be32(spi) || be32(seq_lo)                  (8 bytes), or under SG_ESP_ESN",
                 "          be32(spi) || be32(seq_hi) || be32(seq_lo)  (12 bytes; seq_hi is not on the wire))",
                 "                                    -> P bytes || 16-byte ICV"):
        assert " *   " + line + "\n" in text, line


@pytest.mark.parametrize("open_", (False, True))
def test_argument_errors_before_any_gpu_call(lib, open_):
    from suruga_amd._native import SG_E_ARG, SG_ESP_ESN, SG_ESP_KEEP_FAILED

    call = lib.sg_open_batch_esp if open_ else lib.sg_seal_batch_esp

    def rejected(what, **fields):
        for count in (4, 0):  # the arguments are checked first, also of an empty call
            b = good()
            b.count = count
            for name, v in fields.items():
                setattr(b, name, v)
            assert call(C.byref(b)) == SG_E_ARG, (what, count)
            assert lib.sg_last_error(), what

    assert call(None) == SG_E_ARG and lib.sg_last_error()
    rejected("unknown flags", flags=0x4)
    rejected("unknown flags beside the known", flags=SG_ESP_KEEP_FAILED | 0x80000000)
    for field in ("keys", "salts", "spi", "status", "in_", "out"):
        rejected(f"NULL {field}", **{field: None})
    if open_:
        rejected("open without seq_out", seq_out=None)
        rejected("payload_len without next_header_out", payload_len=0x7000)
        rejected("next_header_out without payload_len", next_header_out=0x7001)
        rejected("ESN without replay_top", flags=SG_ESP_ESN, window=64)
        for w in (0, 2**31 + 1, 0xFFFFFFFF):
            rejected(f"ESN with window {w}", flags=SG_ESP_ESN, replay_top=0x9000, window=w)
        rejected("misaligned replay_top", flags=SG_ESP_ESN, replay_top=0x9004, window=64)
    else:
        rejected("seal without seq", seq=None)
    for field in ("salts", "spi", "sa_index", "len"):
        for o in (1, 2, 3):
            rejected(f"misaligned {field}", **{field: 0x7000 + o}, max_len=1200)
    for o in (1, 2, 3):
        rejected("misaligned payload_len", payload_len=0x7000 + o, next_header_out=0x7101)
    for field in ("seq", "iv", "seq_out", "replay_top", "in_off", "out_off"):
        for o in (1, 2, 4, 7):
            rejected(f"misaligned {field}", **{field: 0x8000 + o})
    rejected("num_sas 0", num_sas=0)
    for a in (0, 1, 2, 3, 5, 6, 18, 255, 257, 260, 512, 0xFFFFFFFC):
        rejected(f"align {a}", align=a)
    rejected("uniform_next_header 256", uniform_next_header=256)
    rejected("uniform_next_header far above", uniform_next_header=0xFFFFFFFF)
    # the bound: open on the packet, seal on 32 + P, which the padding carries beyond the payload's own length
    limit = 16384 if open_ else 16384 - 34
    rejected("uniform_len above the bound", uniform_len=limit + 1)
    rejected("max_len above the bound", len=0x9000, max_len=limit + 1)
    rejected("max_len far above", len=0x9000, max_len=0xFFFFFFFF)
    rejected("max_len whose sum wraps", len=0x9000, max_len=0xFFFFFFFF - 33)
    if not open_:
        assert E.packet_len(16126, 256) == 16384 - 224 and E.packet_len(16127, 256) == 16384 + 32
        rejected("a payload whose padding passes the bound", uniform_len=16127, align=256)
        rejected("... with a length array", len=0x9000, max_len=16127, align=256)


@pytest.mark.parametrize("open_", (False, True))
def test_empty_call_launches_nothing(lib, open_):
    from suruga_amd._native import SG_ESP_ESN, SG_ESP_KEEP_FAILED

    call = lib.sg_open_batch_esp if open_ else lib.sg_seal_batch_esp
    limit = 16384 if open_ else 16384 - 34
    b = good()
    b.count = 0
    assert call(C.byref(b)) == 0
    b.flags, b.uniform_len, b.align = SG_ESP_KEEP_FAILED, limit, 16
    assert call(C.byref(b)) == 0
    b.flags, b.replay_top, b.window = SG_ESP_ESN | SG_ESP_KEEP_FAILED, 0x9000, 2**31
    assert call(C.byref(b)) == 0
    b.window = 1
    assert call(C.byref(b)) == 0
    b.len, b.max_len, b.uniform_len = 0xA000, limit, 0xFFFFFFFF  # with a length array uniform_len is not read
    assert call(C.byref(b)) == 0
    b.align, b.max_len = 256, 16384 if open_ else 16126  # seal: the largest payload whose packet fits at this align
    assert call(C.byref(b)) == 0
    b.payload_len, b.next_header_out, b.sa_index, b.in_off, b.out_off = 0xB000, 0xB401, 0xB100, 0xB200, 0xB300
    b.iv, b.next_header, b.uniform_next_header = 0xB500, 0xB603, 255
    assert call(C.byref(b)) == 0
    if open_:
        b.seq, b.iv, b.next_header = None, None, None  # open reads none of them
    else:
        b.seq_out, b.payload_len, b.replay_top, b.window = None, None, None, 0  # seal reads none: no pairing, no window rule
    assert call(C.byref(b)) == 0


def test_length_functions_against_the_reference(lib):
    for align in (4, 8, 16, 64, 252, 256):
        for n in range(0, 601):
            assert lib.sg_esp_padded_len(n, align) == E.padded_len(n, align), (n, align)
            assert lib.sg_esp_packet_len(n, align) == E.packet_len(n, align) == 32 + E.padded_len(n, align), (n, align)
    assert lib.sg_esp_padded_len(84, 4) == 88 and lib.sg_esp_packet_len(16350, 4) == 16384
    # the ends of 32 bits: nothing wraps
    assert lib.sg_esp_padded_len(0xFFFFFFFA, 4) == 0xFFFFFFFC and lib.sg_esp_padded_len(0xFFFFFFFB, 4) == 0xFFFFFFFF
    assert lib.sg_esp_padded_len(0xFFFFFFFD, 4) == 0xFFFFFFFF and lib.sg_esp_padded_len(0xFFFFFFFF, 256) == 0xFFFFFFFF
    assert lib.sg_esp_packet_len(0xFFFFFFDA, 4) == 0xFFFFFFFC and lib.sg_esp_packet_len(0xFFFFFFDB, 4) == 0xFFFFFFFF
    assert lib.sg_esp_packet_len(0xFFFFFFFF, 4) == 0xFFFFFFFF
    for n in (0xFFFFFF00, 0xFFFFFFDA, 0xFFFFFFFA):
        for align in (4, 16, 256):
            assert lib.sg_esp_padded_len(n, align) == min(E.padded_len(n, align), 0xFFFFFFFF)
    assert lib.sg_esp_padded_len(7, 0) == 9  # an align of 0 divides nothing


def test_seq_hi_against_the_reference(lib):
    rng = random.Random(7634)
    for w in (1, 2, 64, 600, 2**31):
        for tl in (0, w - 2, w - 1, w, 300, 2**32 - 1):
            top = (rng.choice((0, 5, 2**32 - 1)) << 32) | (tl & E.M32)
            for lo in list(range(0, 601)) + [2**32 - 1 - k for k in range(0, 601)]:
                assert lib.sg_esp_seq_hi(top, w, lo) == E.seq_hi(top, w, lo), (hex(top), w, lo)
    for _ in range(20000):
        top, w, lo = rng.randrange(2**64), rng.randrange(1, 2**31 + 1), rng.randrange(2**32)
        assert lib.sg_esp_seq_hi(top, w, lo) == E.seq_hi(top, w, lo) == E.seq_in_window(top, w, lo) >> 32


def test_python_surface(lib):
    import suruga_amd
    from suruga_amd import esp, wg

    assert {"EspBatch", "seal_esp", "open_esp", "esp_padded_len", "esp_packet_len", "esp_seq_hi"} <= set(suruga_amd.__all__)
    assert esp.padded_len(84) == 88 and esp.packet_len(84) == 120 and esp.padded_len(0, 256) == 256
    assert suruga_amd.esp_padded_len(1438, 16) == 1440 and suruga_amd.esp_packet_len(0) == 36
    assert esp.seq_hi(5 << 32 | 100, 64, 36) == 6 == suruga_amd.esp_seq_hi(5 << 32 | 100, 64, 36)
    # WireGuard's helpers keep their names
    assert suruga_amd.padded_len is wg.padded_len and suruga_amd.message_len is wg.message_len
    with pytest.raises(ValueError):
        esp.seal_esp(esp.EspBatch(count=0, keys=None, salts=None, spi=None, inp=None, out=None, status=None))
    with pytest.raises(ValueError):
        esp.open_esp(esp.EspBatch(count=0, keys=None, salts=None, spi=None, inp=None, out=None, status=None))


def test_kernel_file_is_part_of_the_build_and_the_source_hash():
    from suruga_amd import _build

    names = [p.name for p in _build.HIP_SOURCES]
    assert {"sg_esp.hip", "sg_esp_capi.cpp", "sg_esp_host.cpp"} <= set(names)
    assert "sg_esp.h" in [p.name for p in _build.HIP_DEPS]
    # the host-only files stay free of HIP
    for f in ("sg_esp.h", "sg_esp_host.cpp"):
        text = (_build.CSRC / f).read_text()
        assert "hip_runtime" not in text and "__device__" not in text and "__global__" not in text, f
    census = (ROOT / "tools" / "isa_census.py").read_text()
    assert '"sg_esp.hip"' in census
