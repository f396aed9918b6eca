"""DTLS 1.3 records of a device-resident batch, TLS_CHACHA20_POLY1305_SHA256
(``sg_seal_batch_dtls13`` / ``sg_open_batch_dtls13``, RFC 9147 section 4).

One launch seals or opens every record of the call.  Seal takes the content and writes the
record: the unified header (first byte ``001CSLEE``, connection ID, the low 8 or 16 bits of
the sequence number, the optional length), the RFC 8439 ciphertext of content, type byte and
zero padding, the tag; the additional data is that header, the nonce the IV XOR the 64-bit
sequence number, and the sequence number bytes are masked last with a ChaCha20 block under
``sn_key`` whose counter and nonce are the first 16 bytes of ciphertext (section 4.2.3).
Open checks the header's shape, takes the key row from the two epoch bits on the wire,
unmasks the sequence number bytes, rebuilds the 64-bit number against ``expected``,
decrypts, and on a good tag finds the type byte behind the padding; a record that fails its
tag releases neither plaintext nor sequence number.  The handshake, ACKs, the replay window
and ``expected``, the epoch's upper bits, the AEAD limits, datagram parsing and the CID
lookup stay with the caller.

Tensors are torch tensors on the GPU (PyTorch is used here only for device memory and
streams); all arithmetic runs in the gfx950 kernel.  ``header_len``, ``inner_len``,
``record_len`` and ``record_keys`` are the host helpers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _native as N
from ._native import SG_STATUS_BAD_HEADER, SG_STATUS_NO_TYPE  # noqa: F401  (open's two statuses beyond 0..3)
from .batch import _ptr, _stream_handle


@dataclass
class Dtls13Batch:
    """Arguments of one ``sg_*_batch_dtls13`` call (see include/suruga_gpu.h)."""

    count: int
    keys: object                      # uint8 [rows, 32], device: rows = num_conns, or 4 * num_conns with epoch_rows
    ivs: object                       # uint8 [rows, 12], device
    sn_keys: object                   # uint8 [rows, 32], device
    inp: object                       # uint8 device buffer
    out: object                       # uint8 device buffer, not overlapping inp
    status: object                    # uint8 [count] device
    cids: object = None               # seal: uint8 [num_conns, cid_len] device, or None where cid_len is 0
    cid_len: int = 0
    seq: object = None                # seal: uint64 [count] device
    type: object = None               # seal: uint8 [count] device, or None: uniform_type
    uniform_type: int = 23
    epoch: object = None              # seal: uint8 [count] device, or None: uniform_epoch
    uniform_epoch: int = 0
    pad_to: int = 0                   # seal: 0 or 1 none, else the inner plaintext's multiple
    seq16: bool = False               # seal: 16-bit sequence number on the wire
    length: bool = False              # seal: the header carries the length field
    expected: object = None           # open: uint64 [rows] device, highest deprotected number + 1
    seq_out: object = None            # open: uint64 [count] device
    epoch_out: object = None          # open: uint8 [count] device
    content_len: object = None        # open: uint32 [count] device
    type_out: object = None           # open: uint8 [count] device
    key_index: object = None          # uint32 [count] device, or None: connection 0
    epoch_rows: bool = False          # four rows per connection, chosen by the epoch's low two bits
    uniform_len: int = 0
    lens: object = None               # uint32 [count] device, or None
    max_len: int = 0
    in_stride: int = 0
    out_stride: int = 0
    in_off: object = None             # uint64 [count] device, or None
    out_off: object = None
    keep_failed: bool = False         # open: keep the unauthenticated bytes of BAD_MAC records
    stream: object = None             # torch.cuda.Stream / raw handle (0: the NULL stream) / None = current stream

    @property
    def flags(self) -> int:
        return ((N.SG_DTLS13_SEQ16 if self.seq16 else 0) | (N.SG_DTLS13_LENGTH if self.length else 0)
                | (N.SG_DTLS13_EPOCH_ROWS if self.epoch_rows else 0) | (N.SG_DTLS13_KEEP_FAILED if self.keep_failed else 0))

    def to_c(self) -> N.SgDtls13Batch:
        b = N.SgDtls13Batch()
        b.count, b.flags = self.count, self.flags
        b.keys, b.ivs, b.sn_keys, b.cids = _ptr(self.keys), _ptr(self.ivs), _ptr(self.sn_keys), _ptr(self.cids)
        b.key_index, b.seq, b.type, b.epoch = _ptr(self.key_index), _ptr(self.seq), _ptr(self.type), _ptr(self.epoch)
        b.expected, b.seq_out, b.epoch_out = _ptr(self.expected), _ptr(self.seq_out), _ptr(self.epoch_out)
        b.content_len, b.type_out = _ptr(self.content_len), _ptr(self.type_out)
        rows = int(self.keys.numel()) // 32
        b.num_conns = rows // 4 if self.epoch_rows else rows
        b.cid_len, b.pad_to = self.cid_len, self.pad_to
        b.uniform_type, b.uniform_epoch = self.uniform_type, self.uniform_epoch & 0xff
        b.in_, b.in_off, b.in_stride = _ptr(self.inp), _ptr(self.in_off), self.in_stride
        b.out, b.out_off, b.out_stride = _ptr(self.out), _ptr(self.out_off), self.out_stride
        b.len, b.uniform_len, b.max_len = _ptr(self.lens), self.uniform_len, self.max_len
        b.status = _ptr(self.status)
        b.stream = _stream_handle(self.stream)
        return b


def seal_dtls13(batch: Dtls13Batch) -> None:
    """Seal every content: out_i = header || ciphertext || tag, ``record_len(len_i, pad_to,
    flags, cid_len)`` bytes; ``batch.status`` is 0 or 3 (longer than max_len)."""
    if batch.seq is None:
        raise ValueError("seal_dtls13 needs the seq tensor")
    cb = batch.to_c()
    N.check(N.load().sg_seal_batch_dtls13(C.byref(cb)))


def open_dtls13(batch: Dtls13Batch) -> None:
    """Open every record: out_i = the inner plaintext, the 64-bit sequence number in
    ``batch.seq_out``, the epoch bits in ``batch.epoch_out``, the content's length and type in
    ``batch.content_len`` / ``batch.type_out``; ``batch.status`` is 0, 1 (wrong tag: output
    and sequence number zeroed unless keep_failed), 2 (no room for header and tag), 3 (longer
    than max_len), 5 (authentic, but no type byte) or 6 (not a record of this shape)."""
    for name in ("expected", "seq_out", "epoch_out", "content_len", "type_out"):
        if getattr(batch, name) is None:
            raise ValueError(f"open_dtls13 needs the {name} tensor")
    cb = batch.to_c()
    N.check(N.load().sg_open_batch_dtls13(C.byref(cb)))


def _flags(seq16: bool, length: bool) -> int:
    return (N.SG_DTLS13_SEQ16 if seq16 else 0) | (N.SG_DTLS13_LENGTH if length else 0)


def header_len(seq16: bool = False, length: bool = False, cid_len: int = 0) -> int:
    """``sg_dtls13_header_len``: the unified header's bytes.  Host only."""
    return int(N.load().sg_dtls13_header_len(_flags(seq16, length), cid_len))


def inner_len(length: int, pad_to: int = 0) -> int:
    """``sg_dtls13_inner_len``: content, type byte and padding.  Host only."""
    return int(N.load().sg_dtls13_inner_len(length, pad_to))


def record_len(length: int, pad_to: int = 0, seq16: bool = False, with_length: bool = False, cid_len: int = 0) -> int:
    """``sg_dtls13_record_len``: header, inner plaintext and tag, the room a seal needs.  Host only."""
    return int(N.load().sg_dtls13_record_len(length, pad_to, _flags(seq16, with_length), cid_len))


def record_keys(secrets, update: bool = False, threads: int = 8):
    """RFC 9147 section 5.9 / 4.2.3 for many traffic secrets (``sg_dtls13_record_keys``).

    secrets: uint8 [count, 32].  Returns (keys, ivs, sn_keys) as uint8 arrays [count, 32],
    [count, 12] and [count, 32], the tables of ``Dtls13Batch``.  With ``update`` every secret
    takes one "traffic upd" step first and the call returns (keys, ivs, sn_keys,
    next_secrets).  The argument is left as it was."""
    sec = np.array(secrets, dtype=np.uint8, order="C")  # a copy: the C call ratchets in place
    if sec.ndim != 2 or sec.shape[1] != 32:
        raise ValueError("secrets must be [count, 32]")
    count = sec.shape[0]
    keys = np.empty((count, 32), dtype=np.uint8)
    ivs = np.empty((count, 12), dtype=np.uint8)
    sns = np.empty((count, 32), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N.check(N.load().sg_dtls13_record_keys(count, p(sec), p(keys), p(ivs), p(sns), int(bool(update)), threads))
    return (keys, ivs, sns, sec) if update else (keys, ivs, sns)
