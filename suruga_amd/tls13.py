"""TLS 1.3 record layer (RFC 8446 section 5) over the batched GPU path.

The protected stream of a TLS 1.3 connection with TLS_CHACHA20_POLY1305_SHA256:

* ``Tls13Writer.write_data``: ONE ``sg_write_records_tls13`` per call.  The data
  is cut into 2^14-byte fragments; record i is
  ``17 03 03 be16(n + 17) || ct(content || inner_type) || tag`` with
  seq = write_count + i and no padding.
* ``Tls13StreamReader``: one ``sg_read_records_tls13`` per receive buffer.  Every
  complete record is opened and stripped of its inner type and padding;
  ``drain`` returns ``[(inner_type, content)]``.

Key and write IV come from the caller's key schedule, or the library derives
them from the direction's traffic secret (``from_secret``, RFC 8446 section 7.3).
A writer or reader made from a secret follows a KeyUpdate (section 4.6.3, 7.2):
``Tls13Writer.send_key_update`` writes the message and ratchets, and
``Tls13StreamReader.drain`` ratchets where it delivers one, inside one buffer
too.  One made from key and IV cannot, and for it a KeyUpdate is a new writer /
reader.  The plaintext records of the handshake (outer types 20 - 22) are not
part of the protected stream: the caller removes them first.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from .cipher import TlsError, TlsErrorKind, _GpuCtx, _set_iv
from .tls import _ERR_KIND, _sink

APPLICATION_DATA, ALERT, HANDSHAKE = 23, 21, 22
RECORD_MAX_LEN = 1 << 14
KEY_UPDATE = 24  # HandshakeType key_update (RFC 8446 section 4)


def key_update_message(request_update: bool) -> bytes:
    """The KeyUpdate handshake message: 18 00 00 01 || update_not_requested(0) / update_requested(1)."""
    return bytes([KEY_UPDATE, 0, 0, 1, 1 if request_update else 0])


def _is_key_update(inner_type: int, content: bytes) -> bool:
    return inner_type == HANDSHAKE and len(content) == 5 and content[:4] == key_update_message(False)[:4] \
        and content[4] in (0, 1)


class _Tls13Ctx(_GpuCtx):
    """One direction's ``sg_ctx`` with its write IV (RFC 8446 section 5.3)."""

    def __init__(self, key: bytes, iv: bytes, device: int = 0):
        super().__init__(key, device)
        _set_iv(self, iv)

    @classmethod
    def from_secret(cls, secret: bytes, device: int = 0) -> "_Tls13Ctx":
        """Key and IV derived from the traffic secret, which the context keeps (``sg_ctx_set_traffic_secret``)."""
        secret = bytes(secret)
        if len(secret) != 32:
            raise ValueError(f"the traffic secret must be 32 bytes, got {len(secret)}")
        self = cls.__new__(cls)
        _GpuCtx.__init__(self, bytes(N.SG_KEY_LEN), device)  # the derived key replaces this placeholder
        N.check(self._lib.sg_ctx_set_traffic_secret(self._ptr, secret))
        return self

    def key_update(self) -> None:
        N.check(self._lib.sg_ctx_key_update(self._ptr))


class Tls13Writer:
    def __init__(self, sink, key: bytes, iv: bytes, device: int = 0):
        self.writer = sink
        self._write = _sink(sink)
        self.ctx = _Tls13Ctx(key, iv, device)
        self.write_count = 0

    @classmethod
    def from_secret(cls, sink, secret: bytes, device: int = 0) -> "Tls13Writer":
        """A writer under the keys of a traffic secret; it can ``key_update``."""
        self = cls.__new__(cls)
        self.writer = sink
        self._write = _sink(sink)
        self.ctx = _Tls13Ctx.from_secret(secret, device)
        self.write_count = 0
        return self

    def key_update(self) -> None:
        """The next generation's keys (``sg_ctx_key_update``); sequence numbers restart at 0
        (RFC 8446 section 5.3).  Needs a writer made ``from_secret``."""
        self.ctx.key_update()
        self.write_count = 0

    def send_key_update(self, request_update: bool = False) -> None:
        """Writes the KeyUpdate message as a handshake record under the current keys, then
        switches to the next generation (RFC 8446 section 4.6.3)."""
        self.write_data(HANDSHAKE, key_update_message(request_update))
        self.key_update()

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
        self._follows_key_updates = False
        self.key_update_requested = False

    @classmethod
    def from_secret(cls, secret: bytes, device: int = 0, max_records: int = 1 << 16) -> "Tls13StreamReader":
        """A reader under the keys of a traffic secret.  ``drain`` follows the peer's KeyUpdate
        messages: where it delivers one it ratchets, restarts ``read_count`` at 0 and reads on.
        ``key_update_requested`` turns True when one asked for an update in return (the
        caller answers with ``Tls13Writer.send_key_update`` and resets it)."""
        self = cls.__new__(cls)
        self.ctx = _Tls13Ctx.from_secret(secret, device)
        self.read_count = 0
        self.buf = bytearray()
        self.max_records = max_records
        self.types = (C.c_uint8 * max_records)()
        self.lens = (C.c_uint32 * max_records)()
        self._follows_key_updates = True
        self.key_update_requested = False
        return self

    def key_update(self) -> None:
        """The reader's counterpart of ``Tls13Writer.key_update``."""
        self.ctx.key_update()
        self.read_count = 0

    def feed(self, data: bytes) -> None:
        self.buf += data

    def drain(self):
        """-> list of (inner_type, content).  Raises TlsError at the first failing
        record, after consuming the records before it (they are lost to the caller,
        as a connection that saw a fatal alert condition is).

        A reader made ``from_secret`` changes keys where the last record a read
        delivered is a KeyUpdate message: the records behind it, which that read
        stopped at because they fail under the old key, are read again under the
        next generation and appended."""
        msgs = []
        while self.buf:
            got, error = self._read()
            msgs += got
            if self._follows_key_updates and got and _is_key_update(*got[-1]):
                self.key_update()
                self.key_update_requested |= got[-1][1][4] == 1
                continue
            if error != N.SG_OK:
                kind, desc = _ERR_KIND.get(error, (TlsErrorKind.InternalError, f"status {error}"))
                raise TlsError(kind, desc)
            break  # what is left is an incomplete record
        return msgs

    def _read(self):
        """One ``sg_read_records_tls13`` over the buffer: (delivered records, error)."""
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
        return msgs, res.error

    def close(self) -> None:
        self.ctx.close()
