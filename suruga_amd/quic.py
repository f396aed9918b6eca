"""QUIC packet protection of a device-resident batch (``sg_seal_batch_quic`` /
``sg_open_batch_quic``, RFC 9001 section 5.3 - 5.4).

One launch protects or unprotects every packet of the call: AEAD_CHACHA20_POLY1305 with
the packet's own header as additional data and ``iv XOR packet number`` as nonce, then
ChaCha20 header protection; on open the mask comes off first, the packet number is
decoded against the expected one (RFC 9000 appendix A.3) and a packet that fails its tag
releases neither plaintext nor number.  The caller says where each packet lies and where
its packet number field starts; datagram parsing stays with the QUIC stack.

Tensors are torch tensors on the GPU (PyTorch is used here only for device memory and
streams); all arithmetic runs in the gfx950 kernel.  ``decode_pn`` is the host helper.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass

from . import _native as N
from .batch import _ptr, _stream_handle


@dataclass
class QuicBatch:
    """Arguments of one ``sg_*_batch_quic`` call (see include/suruga_gpu.h)."""

    count: int
    keys: object                      # uint8 [num_keys, 32], device
    ivs: object                       # uint8 [num_keys, 12], device
    hp_keys: object                   # uint8 [num_keys, 32], or [num_keys / 2, 32] with key_phase
    pn: object                        # uint64 [count] device: seal the number, open the expected one
    inp: object                       # uint8 device buffer
    out: object                       # uint8 device buffer; must not overlap inp
    status: object                    # uint8 [count] device
    pn_out: object = None             # open: uint64 [count] device
    key_index: object = None          # uint32 [count] device, or None: connection 0
    pn_off: object = None             # uint32 [count] device, or None: uniform_pn_off
    uniform_pn_off: int = 0
    uniform_len: int = 0
    lens: object = None               # uint32 [count] device, or None
    max_len: int = 0
    in_stride: int = 0
    out_stride: int = 0
    in_off: object = None             # uint64 [count] device, or None
    out_off: object = None
    key_phase: bool = False           # keys / ivs hold two generations a connection, rows 2 k + phase
    keep_failed: bool = False         # open: keep the unauthenticated bytes of BAD_MAC packets
    stream: object = None             # torch.cuda.Stream / raw handle (0: the NULL stream) / None = current stream

    def to_c(self) -> N.SgQuicBatch:
        b = N.SgQuicBatch()
        b.count = self.count
        b.flags = (N.SG_QUIC_KEY_PHASE if self.key_phase else 0) | (N.SG_QUIC_KEEP_FAILED if self.keep_failed else 0)
        b.keys, b.ivs, b.hp_keys = _ptr(self.keys), _ptr(self.ivs), _ptr(self.hp_keys)
        b.num_keys = int(self.keys.numel()) // 32
        b.key_index = _ptr(self.key_index)
        b.pn, b.pn_out = _ptr(self.pn), _ptr(self.pn_out)
        b.pn_off, b.uniform_pn_off = _ptr(self.pn_off), self.uniform_pn_off
        b.in_, b.in_off, b.in_stride = _ptr(self.inp), _ptr(self.in_off), self.in_stride
        b.out, b.out_off, b.out_stride = _ptr(self.out), _ptr(self.out_off), self.out_stride
        b.len, b.uniform_len, b.max_len = _ptr(self.lens), self.uniform_len, self.max_len
        b.status = _ptr(self.status)
        b.stream = _stream_handle(self.stream)
        return b


def seal_quic(batch: QuicBatch) -> None:
    """Protect every packet: out_i = protected header || ciphertext || tag, len_i + 16 bytes;
    ``batch.status`` is 0, 2 (no full header protection sample) or 3 (longer than max_len)."""
    cb = batch.to_c()
    N.check(N.load().sg_seal_batch_quic(C.byref(cb)))


def open_quic(batch: QuicBatch) -> None:
    """Unprotect every packet: out_i = header || plaintext, len_i - 16 bytes, the packet number
    in ``batch.pn_out``; ``batch.status`` is 0, 1 (wrong tag: output and number zeroed unless
    keep_failed), 2 (too short) or 3 (longer than max_len)."""
    if batch.pn_out is None:
        raise ValueError("open_quic needs a pn_out tensor")
    cb = batch.to_c()
    N.check(N.load().sg_open_batch_quic(C.byref(cb)))


def decode_pn(expected_pn: int, truncated: int, pn_len: int) -> int:
    """RFC 9000 appendix A.3 (``sg_quic_decode_pn``): the full packet number of ``truncated``
    (``pn_len`` bytes) given ``expected_pn`` = largest received + 1.  Host only."""
    return int(N.load().sg_quic_decode_pn(expected_pn, truncated, pn_len))
