"""WireGuard transport data messages of a device-resident batch (``sg_seal_batch_wg`` /
``sg_open_batch_wg``, whitepaper section 5.4.6).

One launch seals or opens every packet of the call.  Seal takes the inner packet and
writes the message: the 16-byte header (type 4, receiver index, counter), the RFC 8439
ciphertext of the inner packet zero-padded to 16 bytes (at most ``pad_cap``), the tag.
Open checks the header, reads the counter off the wire, decrypts, and on a good tag gives
the inner packet's length from its IPv4 or IPv6 header, so that the padding can be cut
without a look at the plaintext on the host; a message that fails its tag releases neither
plaintext nor counter.  Both work in place with 16 bytes of headroom.  The replay window,
the receiver-index lookup, the allowed-IPs check and the handshake stay with the caller.

Tensors are torch tensors on the GPU (PyTorch is used here only for device memory and
streams); all arithmetic runs in the gfx950 kernel.  ``padded_len`` and ``message_len``
are the host helpers.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _native as N
from ._native import SG_STATUS_BAD_HEADER, SG_STATUS_BAD_INNER  # noqa: F401  (open's two statuses beyond 0..3)
from .batch import _ptr, _stream_handle


@dataclass
class WgBatch:
    """Arguments of one ``sg_*_batch_wg`` call (see include/suruga_gpu.h)."""

    count: int
    keys: object                      # uint8 [num_keys, 32], device: one row per session direction
    inp: object                       # uint8 device buffer
    out: object                       # uint8 device buffer; in place: seal out + 16 == inp, open out == inp + 16
    status: object                    # uint8 [count] device
    receiver: object = None           # seal: uint32 [num_keys] device, the index written into the header
    counter: object = None            # seal: uint64 [count] device
    counter_out: object = None        # open: uint64 [count] device
    inner_len: object = None          # open: uint32 [count] device, or None: nothing parsed
    key_index: object = None          # uint32 [count] device, or None: row 0
    pad_cap: int = 0                  # seal: 0, or the bound of the padded length (the MTU)
    uniform_len: int = 0
    lens: object = None               # uint32 [count] device, or None
    max_len: int = 0
    in_stride: int = 0
    out_stride: int = 0
    in_off: object = None             # uint64 [count] device, or None
    out_off: object = None
    keep_failed: bool = False         # open: keep the unauthenticated bytes of BAD_MAC packets
    stream: object = None             # torch.cuda.Stream / raw handle (0: the NULL stream) / None = current stream

    def to_c(self) -> N.SgWgBatch:
        b = N.SgWgBatch()
        b.count = self.count
        b.flags = N.SG_WG_KEEP_FAILED if self.keep_failed else 0
        b.keys, b.receiver, b.key_index = _ptr(self.keys), _ptr(self.receiver), _ptr(self.key_index)
        b.num_keys, b.pad_cap = int(self.keys.numel()) // 32, self.pad_cap
        b.counter, b.counter_out, b.inner_len = _ptr(self.counter), _ptr(self.counter_out), _ptr(self.inner_len)
        b.in_, b.in_off, b.in_stride = _ptr(self.inp), _ptr(self.in_off), self.in_stride
        b.out, b.out_off, b.out_stride = _ptr(self.out), _ptr(self.out_off), self.out_stride
        b.len, b.uniform_len, b.max_len = _ptr(self.lens), self.uniform_len, self.max_len
        b.status = _ptr(self.status)
        b.stream = _stream_handle(self.stream)
        return b


def seal_wg(batch: WgBatch) -> None:
    """Seal every inner packet: out_i = header || ciphertext || tag, ``message_len(len_i,
    pad_cap)`` bytes; ``batch.status`` is 0 or 3 (longer than max_len)."""
    if batch.receiver is None or batch.counter is None:
        raise ValueError("seal_wg needs the receiver and counter tensors")
    cb = batch.to_c()
    N.check(N.load().sg_seal_batch_wg(C.byref(cb)))


def open_wg(batch: WgBatch) -> None:
    """Open every message: out_i = the padded inner packet, len_i - 32 bytes, the counter in
    ``batch.counter_out`` and the inner packet's length in ``batch.inner_len``;
    ``batch.status`` is 0, 1 (wrong tag: output and counter zeroed unless keep_failed), 2 (shorter
    than 32 bytes), 3 (longer than max_len), 6 (not a type 4 message) or 7 (authentic, but the
    inner IP header's length does not fit)."""
    if batch.counter_out is None:
        raise ValueError("open_wg needs a counter_out tensor")
    cb = batch.to_c()
    N.check(N.load().sg_open_batch_wg(C.byref(cb)))


def padded_len(length: int, pad_cap: int = 0) -> int:
    """``sg_wg_padded_len``: the AEAD's plaintext length of an inner packet.  Host only."""
    return int(N.load().sg_wg_padded_len(length, pad_cap))


def message_len(length: int, pad_cap: int = 0) -> int:
    """``sg_wg_message_len``: 32 + ``padded_len``, the room a seal needs.  Host only."""
    return int(N.load().sg_wg_message_len(length, pad_cap))
