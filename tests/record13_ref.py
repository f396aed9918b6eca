"""The record layer in TLS 1.3 and RFC 7905 restated for the tests -- TEST
INFRASTRUCTURE ONLY.

Streams are built from tests/tls13_ref.py (``seal(..., pad=...)``, tied to OpenSSL
by tests/golden/tls13_records.json) and tests/rfc8439_ref.py (RFC 7905: the TLS
1.2 record of tests/golden/rfc7905_records.json), with the result a read of them
must give: the delivered types, lengths and bytes and ``records``, ``consumed``,
``out_len`` and ``error`` of sg_read_result.  tests/test_record13_ref.py pins both
against the golden files.

* ``Item``: one record of a stream -- its content, type and padding, or one of
  the failing kinds, each composed as data: ``tag`` (a tag bit flipped ->
  BAD_MAC), ``zeros`` (an authentic all-zero inner plaintext -> UNEXPECTED_MESSAGE,
  RFC 8446 section 5.4) and ``long`` (authentic content of 2^14 + 1 bytes ->
  RECORD_OVERFLOW).
* ``stream13`` / ``stream7905``: the wire bytes and every record's offset.
* ``expected_read``: what the reader delivers: everything before the first
  failing record, and that record's error.
* ``gather_model`` / ``gather_check``: the device step of the TLS 1.3 read
  (sg_gather_kernel): prefix, ``ok``, the cursor chain and its sticky stop, as
  whole-buffer images over a sentinel.

Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
import struct
from dataclasses import dataclass, field

import numpy as np

import footprint as fp
import rfc8439_ref as R
import tls13_ref as T

OK, E_BAD_MAC, E_SHORT, E_UNEXPECTED_MESSAGE, E_RECORD_OVERFLOW = 0, 1, 2, 3, 4
FULL = 1 << 14
CHUNK = 256                      # records per pipeline chunk (sg_wire.h kChunk)
PITCH13 = 5 + FULL + 17          # a full TLS 1.3 record on the wire
PITCH12 = 5 + FULL + 16          # a full TLS 1.2 record (draft and RFC 7905)
KEY = hashlib.shake_256(b"record13 key").digest(32)
IV = hashlib.shake_256(b"record13 iv").digest(12)


def content(n: int, tag: str = "") -> bytes:
    return hashlib.shake_256(f"record13 content {tag} {n}".encode()).digest(n) if n else b""


def wire_bound13(n: int) -> int:
    return n + 22 * ((n + FULL - 1) // FULL)


@dataclass
class Item:
    content: bytes
    ctype: int = 23
    pad: int = 0
    fail: str | None = None      # None, "tag", "zeros", "long"
    version: tuple = (3, 3)      # RFC 7905 streams: the record's version bytes

    @property
    def error(self) -> int:
        return {None: OK, "tag": E_BAD_MAC, "zeros": E_UNEXPECTED_MESSAGE, "long": E_RECORD_OVERFLOW}[self.fail]


def failing(kind: str, tag: str = "f") -> Item:
    """A record that stops the reader, composed as data."""
    if kind == "tag":
        return Item(content(100, tag), fail="tag")
    if kind == "zeros":
        return Item(b"", fail="zeros")
    assert kind == "long"
    return Item(content(FULL + 1, tag), fail="long")


@dataclass
class Stream:
    wire: bytes
    offsets: list = field(default_factory=list)   # of every record's header; one more: the end
    items: list = field(default_factory=list)


def record13(key: bytes, iv: bytes, seq: int, it: Item) -> bytes:
    if it.fail == "zeros":
        frag = T.seal_inner(key, iv, seq, bytes(len(it.content) + 1 + it.pad))
    else:
        frag = T.seal(key, iv, seq, it.content, it.ctype, it.pad)
    if it.fail == "tag":
        frag = frag[:-1] + bytes([frag[-1] ^ 0x80])
    return T.header(len(frag)) + frag


def record7905(key: bytes, iv: bytes, seq: int, it: Item) -> bytes:
    ad = struct.pack(">QBBBH", seq, it.ctype, it.version[0], it.version[1], len(it.content))
    frag = R.seal(key, T.nonce(iv, seq), it.content, ad)
    if it.fail == "tag":
        frag = frag[:-1] + bytes([frag[-1] ^ 0x80])
    return struct.pack(">BBBH", it.ctype, it.version[0], it.version[1], len(frag)) + frag


def _stream(make, key, iv, seq0, items, cut):
    parts, offs, pos = [], [], 0
    for i, it in enumerate(items):
        rec = make(key, iv, seq0 + i, it)
        offs.append(pos)
        parts.append(rec)
        pos += len(rec)
    offs.append(pos)
    wire = b"".join(parts)
    return Stream(wire[:len(wire) - cut] if cut else wire, offs, list(items))


def stream13(items, key: bytes = KEY, iv: bytes = IV, seq0: int = 0, cut: int = 0) -> Stream:
    """The TLS 1.3 wire of `items`; cut > 0 drops that many bytes of the last record
    (an incomplete record at the end of the receive buffer)."""
    return _stream(record13, key, iv, seq0, items, cut)


def stream7905(items, key: bytes = KEY, iv: bytes = IV, seq0: int = 0, cut: int = 0) -> Stream:
    return _stream(record7905, key, iv, seq0, items, cut)


@dataclass
class Read:
    types: list
    lens: list
    out: bytes
    records: int
    consumed: int
    out_len: int
    error: int


def expected_read(st: Stream) -> Read:
    """What a read of the whole stream gives: the complete records before the first
    failing one are delivered; an incomplete last record is not an error."""
    types, lens, out = [], [], []
    n, error = 0, OK
    for i, it in enumerate(st.items):
        if st.offsets[i + 1] > len(st.wire):
            break  # incomplete
        if it.fail:
            error = it.error
            break
        types.append(it.ctype)
        lens.append(len(it.content))
        out.append(it.content)
        n += 1
    data = b"".join(out)
    return Read(types, lens, data, n, st.offsets[n], len(data), error)


def out_capacity13(st: Stream) -> int:
    """The out_cap the TLS 1.3 read asks for: the sum of flen - 17 over the complete
    records with flen >= 17."""
    total = 0
    for i in range(len(st.items)):
        if st.offsets[i + 1] > len(st.wire):
            break
        flen = st.offsets[i + 1] - st.offsets[i] - 5
        total += max(flen - 17, 0)
    return total


# ---------------------------------------------------------------------------
# the gather step (sg_gather_kernel / sg_gather_records)
# ---------------------------------------------------------------------------
@dataclass
class Cursor:
    offset: int = 0
    stopped: int = 0


def gather_model(src: np.ndarray, stride: int, status, lens, dst: np.ndarray, dst_off: int, cur: Cursor,
                 use_base: bool):
    """One chunk: returns (image of dst afterwards, next cursor, (ok, bytes)).
    ok: the first record with a status other than 0 or content above 2^14 (count if
    none; 0 if the incoming cursor has stopped); the contents of the records before
    it land back to back at dst_off (+ cur.offset with use_base); no other byte of
    dst changes."""
    count = len(lens)
    ok = count
    for i in range(count):
        if status[i] != 0 or lens[i] > FULL:
            ok = i
            break
    if cur.stopped:
        ok = 0
    img = dst.copy()
    pos = dst_off + (cur.offset if use_base else 0)
    total = 0
    for i in range(ok):
        n = int(lens[i])
        img[pos + total:pos + total + n] = src[i * stride:i * stride + n]
        total += n
    return img, Cursor(cur.offset + total, 1 if (cur.stopped or ok < count) else 0), (ok, total)


def gather_check(got_dst: np.ndarray, got_cur, got_res, want_dst: np.ndarray, want_cur: Cursor, want_res):
    """Whole-buffer comparison and the two small results; raises AssertionError."""
    d = fp.first_diff(got_dst, want_dst)
    assert d is None, f"gather image differs: {d}"
    assert tuple(got_cur) == (want_cur.offset, want_cur.stopped), (tuple(got_cur), want_cur)
    assert tuple(got_res) == tuple(want_res), (tuple(got_res), want_res)
