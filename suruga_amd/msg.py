"""One long device-resident message (``sg_seal_msg_dev`` / ``sg_open_msg_dev``).

``Encryptor::encrypt`` / ``Decryptor::decrypt`` take data and additional data
of any length (cipher/mod.rs:22-32).  The record paths bound a record at 32 KiB
and its AD at 255 bytes; this module is the path beside them: one key, one
nonce, up to ``SG_MSG_MAX_LEN`` bytes of data and of AD, sealed or opened by a
persistent grid over all CUs (suruga_amd/csrc/sg_msg.hip).  Many such
messages go through one call with ``seal_msgs`` / ``open_msgs``
(``sg_seal_msg_batch`` / ``sg_open_msg_batch``, sg_msg_batch.hip): one grid
over the tiles of all messages, one finish launch for all tags.

Two constructions: the draft every other path of the library speaks (8-byte
nonce, the default), and with ``rfc8439=True`` RFC 8439 (12-byte nonce, the
padded MAC stream; ``SG_MSG_RFC8439``) -- what OpenSSL, libsodium's ``_ietf``
form, TLS 1.3, QUIC and WireGuard compute.

Tensors are torch uint8 tensors on the GPU (PyTorch is used only for device
memory and streams); all arithmetic runs in the gfx950 kernels.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional

from . import _native as N
from .batch import _ptr, _stream_handle


def _flags(keep_failed: bool, rfc8439: bool) -> int:
    return (N.SG_MSG_KEEP_FAILED if keep_failed else 0) | (N.SG_MSG_RFC8439 if rfc8439 else 0)


def _nonce(nonce: bytes, rfc8439: bool):
    """(nonce_hi or None, the 8 bytes of ``nonce``): the draft takes 8 bytes
    (chacha20.rs:27), RFC 8439 takes 12 and splits them 4 + 8."""
    nonce = bytes(nonce)
    want = N.SG_RFC8439_NONCE_LEN if rfc8439 else N.SG_NONCE_LEN
    if len(nonce) != want:
        raise ValueError(f"nonce must be {want} bytes, got {len(nonce)}")
    return (nonce[:4], nonce[4:]) if rfc8439 else (None, nonce)


def plan_for(n: int, adlen: int, groups: int = 0, rfc8439: bool = False) -> dict:
    """The launch geometry ``sg_msg_plan_for`` (``sg_msg_plan_for_flags`` with
    ``rfc8439``) computes (host only, no GPU): ``mac_blocks``, ``tiles``,
    ``zero_blocks``, ``tile_blocks``, ``tile_bytes``, ``groups``,
    ``tiles_per_group``.  Raises NativeError above SG_MSG_MAX_LEN."""
    p = N.SgMsgPlan()
    if rfc8439:
        rc = N.load().sg_msg_plan_for_flags(n, adlen, N.SG_MSG_RFC8439, groups, C.byref(p))
    else:
        rc = N.load().sg_msg_plan_for(n, adlen, groups, C.byref(p))
    if rc != N.SG_OK:
        raise N.NativeError(rc, "sg_msg_plan_for: a length above SG_MSG_MAX_LEN")
    return {name: int(getattr(p, name)) for name, _ in N.SgMsgPlan._fields_}


def set_groups(n: int) -> int:
    """``sg_set_msg_groups``: 0 = automatic grid, negative = query; returns the previous setting."""
    return int(N.load().sg_set_msg_groups(n))


def workspace_size() -> int:
    return int(N.load().sg_msg_workspace_size())


def _msg(key, nonce: bytes, ad, inp, in_len, out, status, keep_failed, stream, workspace, rfc8439=False) -> N.SgMsg:
    hi, nonce = _nonce(nonce, rfc8439)
    m = N.SgMsg()
    m.key = _ptr(key)
    m.nonce[:] = nonce
    if hi is not None:
        m.nonce_hi[:] = hi
    m.ad = _ptr(ad)
    m.ad_len = int(ad.numel()) if ad is not None else 0
    m.in_ = _ptr(inp)
    m.in_len = int(inp.numel()) if in_len is None else in_len
    m.out = _ptr(out)
    m.status = _ptr(status)
    m.flags = _flags(keep_failed, rfc8439)
    m.stream = _stream_handle(stream)
    m.workspace = _ptr(workspace)
    m.workspace_size = int(workspace.numel()) if workspace is not None else 0
    return m


@dataclass
class MsgItem:
    """One message of a batch (``struct sg_msg_item``): device tensors, an 8-byte
    nonce (12 bytes in a call with ``rfc8439``), an index into the call's key table.  ``in_len`` defaults to all of
    ``inp`` (seal: n, open: n + 16); ``out`` may be ``inp`` itself."""

    key_index: int
    nonce: bytes
    inp: object
    out: object
    ad: object = None
    in_len: Optional[int] = None
    ad_len: Optional[int] = None


def batch_workspace_size(count: int) -> int:
    return int(N.load().sg_msg_batch_workspace_size(count))


def batch_plan_for(lengths, adlens, groups: int = 0, rfc8439: bool = False) -> dict:
    """The plan ``sg_msg_batch_plan_for`` (``sg_msg_batch_plan_for_flags`` with
    ``rfc8439``) computes (host only, no GPU) for
    messages of ``lengths`` data bytes and ``adlens`` AD bytes: the header
    fields (``tiles``, ``tiles_per_group``, ``groups``, ``segments``,
    ``tile_blocks``, ``tile_bytes``), ``msgs`` (the per-message plans, as
    ``plan_for``), ``segs`` (dicts of msg, tile_begin, tile_end, group),
    ``group_segs`` and ``msg_segs`` ((first, count) runs of ``segs``).  Raises
    NativeError for a length above SG_MSG_MAX_LEN."""
    count = len(lengths)
    if len(adlens) != count:
        raise ValueError("lengths and adlens differ in length")
    n = (C.c_uint64 * max(count, 1))(*lengths)
    a = (C.c_uint64 * max(count, 1))(*adlens)
    plan = N.SgMsgBatchPlan()
    msgs = (N.SgMsgPlan * max(count, 1))()
    cap = N.SG_MSG_MAX_GROUPS + count
    segs = (N.SgMsgSeg * cap)()
    gsp = (N.SgMsgSpan * N.SG_MSG_MAX_GROUPS)()
    msp = (N.SgMsgSpan * max(count, 1))()
    if rfc8439:
        rc = N.load().sg_msg_batch_plan_for_flags(n, a, count, N.SG_MSG_RFC8439, groups, C.byref(plan), msgs, segs, cap,
                                                  gsp, msp)
    else:
        rc = N.load().sg_msg_batch_plan_for(n, a, count, groups, C.byref(plan), msgs, segs, cap, gsp, msp)
    if rc != N.SG_OK:
        raise N.NativeError(rc, "sg_msg_batch_plan_for: a length above SG_MSG_MAX_LEN or too many messages")
    out = {name: int(getattr(plan, name)) for name, _ in N.SgMsgBatchPlan._fields_}
    out["msgs"] = [{name: int(getattr(msgs[i], name)) for name, _ in N.SgMsgPlan._fields_} for i in range(count)]
    out["segs"] = [{name: int(getattr(segs[i], name)) for name, _ in N.SgMsgSeg._fields_}
                   for i in range(out["segments"])]
    out["group_segs"] = [(int(gsp[g].first), int(gsp[g].count)) for g in range(out["groups"])]
    out["msg_segs"] = [(int(msp[i].first), int(msp[i].count)) for i in range(count)]
    return out


def _msg_batch(keys, items, status, keep_failed, stream, workspace, rfc8439=False) -> N.SgMsgBatch:
    arr = (N.SgMsgItem * max(len(items), 1))()
    for d, it in zip(arr, items):
        hi, nonce = _nonce(it.nonce, rfc8439)
        d.key_index = it.key_index
        d.nonce[:] = nonce
        if hi is not None:
            d.nonce_hi[:] = hi
        d.ad = _ptr(it.ad)
        d.ad_len = (int(it.ad.numel()) if it.ad is not None else 0) if it.ad_len is None else it.ad_len
        d.in_ = _ptr(it.inp)
        d.in_len = (int(it.inp.numel()) if it.inp is not None else 0) if it.in_len is None else it.in_len
        d.out = _ptr(it.out)
    b = N.SgMsgBatch()
    b.count = len(items)
    b.flags = _flags(keep_failed, rfc8439)
    b.keys = _ptr(keys)
    b.num_keys = int(keys.shape[0]) if keys is not None else 0
    b.items = arr  # (the struct keeps the array alive)
    b.status = _ptr(status)
    b.stream = _stream_handle(stream)
    b.workspace = _ptr(workspace)
    b.workspace_size = int(workspace.numel()) if workspace is not None else 0
    return b


def seal_msgs(keys, items, stream=None, workspace=None, rfc8439: bool = False) -> None:
    """``sg_seal_msg_batch``: every item's out[0, n + 16) = ct || tag under
    keys[item.key_index] (uint8 [num_keys, 32] on the device), all messages on
    one grid.  Messages must not overlap one another (not checked).
    ``rfc8439``: the whole call in RFC 8439, every nonce 12 bytes."""
    b = _msg_batch(keys, items, None, False, stream, workspace, rfc8439)
    N.check(N.load().sg_seal_msg_batch(C.byref(b)))


def open_msgs(keys, items, status, keep_failed=False, stream=None, workspace=None, rfc8439: bool = False) -> None:
    """``sg_open_msg_batch``: status[i] (device uint8, one per item) becomes 0,
    SG_E_BAD_MAC or SG_E_SHORT (fewer than 16 input bytes: that output is left
    untouched); a failed message's output is zeroed on the device unless
    ``keep_failed``."""
    if status is None:
        raise ValueError("open needs a status tensor")
    b = _msg_batch(keys, items, status, keep_failed, stream, workspace, rfc8439)
    N.check(N.load().sg_open_msg_batch(C.byref(b)))


def seal_msg(key, nonce: bytes, inp, out, ad=None, in_len=None, stream=None, workspace=None,
             rfc8439: bool = False) -> None:
    """out[0, n + 16) = ct || tag of the n = ``in_len`` (default: all of ``inp``)
    bytes of ``inp`` (chacha20_poly1305.rs:48-59).  ``out`` may be ``inp`` itself.
    ``rfc8439``: RFC 8439 with a 12-byte nonce instead of the draft with its 8."""
    m = _msg(key, nonce, ad, inp, in_len, out, None, False, stream, workspace, rfc8439)
    N.check(N.load().sg_seal_msg_dev(C.byref(m)))


def open_(key, nonce: bytes, inp, out, status, ad=None, in_len=None, keep_failed=False, stream=None,
          workspace=None, rfc8439: bool = False) -> int:
    """Open ct || tag (``in_len`` bytes of ``inp``); the MAC result lands in the
    device byte ``status`` (0 ok, 1 BadRecordMac "wrong mac"), and the output of a
    failed open is zeroed on the device unless ``keep_failed``.  Returns SG_OK, or
    SG_E_SHORT for fewer than 16 bytes (nothing is touched then)."""
    if status is None:
        raise ValueError("open needs a status tensor")
    m = _msg(key, nonce, ad, inp, in_len, out, status, keep_failed, stream, workspace, rfc8439)
    return N.check(N.load().sg_open_msg_dev(C.byref(m)))
