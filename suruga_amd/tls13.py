"""TLS 1.3 record layer (RFC 8446 section 5) over the batched GPU path.

The protected stream of a TLS 1.3 connection with TLS_CHACHA20_POLY1305_SHA256:

* ``Tls13Writer.write_data``: ONE ``sg_write_records_tls13`` per call.  The data
  is cut into 2^14-byte fragments; record i is
  ``17 03 03 be16(n + 17) || ct(content || inner_type) || tag`` with
  seq = write_count + i and no padding.
* ``Tls13StreamReader``: one ``sg_read_records_tls13`` per receive buffer.  Every
  complete record is opened and stripped of its inner type and padding;
  ``drain`` returns ``[(inner_type, content)]``.

Key and write IV come from the caller's key schedule; a KeyUpdate is a new
writer / reader.  The plaintext records of the handshake (outer types 20 - 22)
are not part of the protected stream: the caller removes them first.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from .cipher import TlsError, TlsErrorKind, _GpuCtx, _set_iv
from .tls import _ERR_KIND, _sink

APPLICATION_DATA, ALERT, HANDSHAKE = 23, 21, 22
RECORD_MAX_LEN = 1 << 14


class _Tls13Ctx(_GpuCtx):
    """One direction's ``sg_ctx`` with its write IV (RFC 8446 section 5.3)."""

    def __init__(self, key: bytes, iv: bytes, device: int = 0):
        super().__init__(key, device)
        _set_iv(self, iv)


class Tls13Writer:
    def __init__(self, sink, key: bytes, iv: bytes, device: int = 0):
        self.writer = sink
        self._write = _sink(sink)
        self.ctx = _Tls13Ctx(key, iv, device)
        self.write_count = 0

    def write_data(self, inner_type: int, data: bytes) -> None:
        if not 0 < int(inner_type) < 256:
            raise ValueError("the inner content type must be 1..255 (a zero byte reads as padding)")
        if len(data) == 0:
            return  # no record, as TlsWriter.write_data
        lib = N.load()
        wire = (C.c_uint8 * lib.sg_wire_bound_tls13(len(data)))()
        wl = C.c_size_t(0)
        src = (C.c_uint8 * len(data)).from_buffer(data) if isinstance(data, bytearray) else \
            (C.c_uint8 * len(data)).from_buffer_copy(data)
        nrec = N.check(lib.sg_write_records_tls13(self.ctx._ptr, self.write_count, int(inner_type), src, len(data),
                                                  wire, len(wire), C.byref(wl)))
        self._write(bytes(memoryview(wire)[:wl.value]))
        self.write_count += nrec

    def write_application_data(self, data: bytes) -> None:
        self.write_data(APPLICATION_DATA, data)

    def write_alert(self, level: int, description: int) -> None:
        self.write_data(ALERT, bytes([level, description]))

    def close(self) -> None:
        self.ctx.close()


class Tls13StreamReader:
    """Batched reader over a byte stream: ``feed`` the received bytes, ``drain``
    opens every complete buffered record."""

    def __init__(self, key: bytes, iv: bytes, device: int = 0, max_records: int = 1 << 16):
        self.ctx = _Tls13Ctx(key, iv, device)
        self.read_count = 0
        self.buf = bytearray()
        self.max_records = max_records
        self.types = (C.c_uint8 * max_records)()
        self.lens = (C.c_uint32 * max_records)()

    def feed(self, data: bytes) -> None:
        self.buf += data

    def drain(self):
        """-> list of (inner_type, content).  Raises TlsError at the first failing
        record, after consuming the records before it (they are lost to the caller,
        as a connection that saw a fatal alert condition is)."""
        if not self.buf:
            return []
        lib = N.load()
        src = (C.c_uint8 * len(self.buf)).from_buffer(self.buf)
        out = (C.c_uint8 * max(len(self.buf), 1))()
        res = N.SgReadResult()
        N.check(lib.sg_read_records_tls13(self.ctx._ptr, self.read_count, src, len(self.buf), out, len(out),
                                          self.types, self.lens, self.max_records, C.byref(res)))
        del src
        msgs, pos = [], 0
        for i in range(res.records):
            n = self.lens[i]
            msgs.append((int(self.types[i]), bytes(memoryview(out)[pos:pos + n])))
            pos += n
        del self.buf[:res.consumed]
        self.read_count += res.records
        if res.error != N.SG_OK:
            kind, desc = _ERR_KIND.get(res.error, (TlsErrorKind.InternalError, f"status {res.error}"))
            raise TlsError(kind, desc)
        return msgs

    def close(self) -> None:
        self.ctx.close()
