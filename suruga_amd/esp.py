"""IPsec ESP packets of a device-resident batch, ChaCha20-Poly1305 (``sg_seal_batch_esp`` /
``sg_open_batch_esp``, RFC 7634 over RFC 4303).

One launch seals or opens every packet of the call.  Seal takes the payload and writes the
packet: the 16-byte header (SPI, low half of the sequence number, IV), the RFC 8439
ciphertext of payload, padding 1, 2, 3 .., pad length and next header, the ICV; the
additional data is SPI and sequence number, under ``esn`` with the high half that is not
on the wire.  Open checks the SPI, reads sequence number and IV off the wire, infers the
high half from the top of the SA's replay window (RFC 4303 appendix A2.1), decrypts, and
on a good ICV checks the padding and gives the payload's length and the next header, so
that the trailer can be cut without a look at the plaintext on the host; a packet that
fails its ICV releases neither plaintext nor sequence number.  Both work in place with 16
bytes of headroom.  The SPI lookup, the replay window and its top, sequence overflow and
rekeying, TFC padding, the mode, UDP encapsulation and IKE stay with the caller.

Tensors are torch tensors on the GPU (PyTorch is used here only for device memory and
streams); all arithmetic runs in the gfx950 kernel.  ``padded_len``, ``packet_len`` and
``seq_hi`` are the host helpers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _native as N
from ._native import SG_STATUS_BAD_HEADER, SG_STATUS_BAD_INNER  # noqa: F401  (open's two statuses beyond 0..3)
from .batch import _ptr, _stream_handle


@dataclass
class EspBatch:
    """Arguments of one ``sg_*_batch_esp`` call (see include/suruga_gpu.h)."""

    count: int
    keys: object                      # uint8 [num_sas, 32], device: one row per SA and direction
    salts: object                     # uint8 [num_sas, 4], device
    spi: object                       # uint32 [num_sas], device
    inp: object                       # uint8 device buffer
    out: object                       # uint8 device buffer; in place: seal out + 16 == inp, open out == inp + 16
    status: object                    # uint8 [count] device
    seq: object = None                # seal: uint64 [count] device
    iv: object = None                 # seal: uint64 [count] device, or None: the sequence number
    next_header: object = None        # seal: uint8 [count] device, or None: uniform_next_header
    uniform_next_header: int = 0
    align: int = 4                    # seal: payload, padding and trailer end on a multiple of it (4..256)
    seq_out: object = None            # open: uint64 [count] device
    payload_len: object = None        # open: uint32 [count] device, or None: no trailer parse
    next_header_out: object = None    # open: uint8 [count] device, with payload_len
    replay_top: object = None         # open with esn: uint64 [num_sas] device, the top of each SA's window
    window: int = 0                   # open with esn: the window's size, 1..2^31
    sa_index: object = None           # uint32 [count] device, or None: row 0
    esn: bool = False                 # extended sequence numbers
    uniform_len: int = 0
    lens: object = None               # uint32 [count] device, or None
    max_len: int = 0
    in_stride: int = 0
    out_stride: int = 0
    in_off: object = None             # uint64 [count] device, or None
    out_off: object = None
    keep_failed: bool = False         # open: keep the unauthenticated bytes of BAD_MAC packets
    stream: object = None             # torch.cuda.Stream / raw handle (0: the NULL stream) / None = current stream

    def to_c(self) -> N.SgEspBatch:
        b = N.SgEspBatch()
        b.count = self.count
        b.flags = (N.SG_ESP_ESN if self.esn else 0) | (N.SG_ESP_KEEP_FAILED if self.keep_failed else 0)
        b.keys, b.salts, b.spi, b.sa_index = _ptr(self.keys), _ptr(self.salts), _ptr(self.spi), _ptr(self.sa_index)
        b.seq, b.iv, b.next_header = _ptr(self.seq), _ptr(self.iv), _ptr(self.next_header)
        b.seq_out, b.payload_len, b.next_header_out = _ptr(self.seq_out), _ptr(self.payload_len), _ptr(self.next_header_out)
        b.replay_top, b.window = _ptr(self.replay_top), self.window
        b.num_sas, b.align, b.uniform_next_header = int(self.keys.numel()) // 32, self.align, self.uniform_next_header
        b.in_, b.in_off, b.in_stride = _ptr(self.inp), _ptr(self.in_off), self.in_stride
        b.out, b.out_off, b.out_stride = _ptr(self.out), _ptr(self.out_off), self.out_stride
        b.len, b.uniform_len, b.max_len = _ptr(self.lens), self.uniform_len, self.max_len
        b.status = _ptr(self.status)
        b.stream = _stream_handle(self.stream)
        return b


def seal_esp(batch: EspBatch) -> None:
    """Seal every payload: out_i = header || ciphertext || ICV, ``packet_len(len_i, align)``
    bytes; ``batch.status`` is 0 or 3 (longer than max_len)."""
    if batch.seq is None:
        raise ValueError("seal_esp needs the seq tensor")
    cb = batch.to_c()
    N.check(N.load().sg_seal_batch_esp(C.byref(cb)))


def open_esp(batch: EspBatch) -> None:
    """Open every packet: out_i = payload, padding and trailer, len_i - 32 bytes, the 64-bit
    sequence number in ``batch.seq_out``, the payload's length in ``batch.payload_len`` and the
    next header in ``batch.next_header_out``; ``batch.status`` is 0, 1 (wrong ICV: output and
    sequence number zeroed unless keep_failed), 2 (shorter than 34 bytes), 3 (longer than
    max_len), 6 (not the SA's SPI) or 7 (authentic, but the padding is not 1, 2, 3 ..)."""
    if batch.seq_out is None:
        raise ValueError("open_esp needs a seq_out tensor")
    if (batch.payload_len is None) != (batch.next_header_out is None):
        raise ValueError("open_esp takes payload_len and next_header_out together")
    cb = batch.to_c()
    N.check(N.load().sg_open_batch_esp(C.byref(cb)))


def padded_len(length: int, align: int = 4) -> int:
    """``sg_esp_padded_len``: the AEAD's plaintext length of a payload, trailer included.  Host only."""
    return int(N.load().sg_esp_padded_len(length, align))


def packet_len(length: int, align: int = 4) -> int:
    """``sg_esp_packet_len``: 32 + ``padded_len``, the room a seal needs.  Host only."""
    return int(N.load().sg_esp_packet_len(length, align))


def seq_hi(top: int, window: int, seq_lo: int) -> int:
    """``sg_esp_seq_hi``: the high half the open infers for ``seq_lo`` (RFC 4303 appendix A2.1).  Host only."""
    return int(N.load().sg_esp_seq_hi(top, window, seq_lo))
