"""One long device-resident message (``sg_seal_msg_dev`` / ``sg_open_msg_dev``).

``Encryptor::encrypt`` / ``Decryptor::decrypt`` take data and additional data
of any length (cipher/mod.rs:22-32).  The record paths bound a record at 32 KiB
and its AD at 255 bytes; this module is the path beside them: one key, one
nonce, up to ``SG_MSG_MAX_LEN`` bytes of data and of AD, sealed or opened by a
persistent grid over all CUs (suruga_amd/csrc/sg_msg.hip).

Tensors are torch uint8 tensors on the GPU (PyTorch is used only for device
memory and streams); all arithmetic runs in the gfx950 kernels.
"""
from __future__ import annotations

import ctypes as C

from . import _native as N
from .batch import _ptr, _stream_handle


def plan_for(n: int, adlen: int, groups: int = 0) -> dict:
    """The launch geometry ``sg_msg_plan_for`` computes (host only, no GPU):
    ``mac_blocks``, ``tiles``, ``zero_blocks``, ``tile_blocks``, ``tile_bytes``,
    ``groups``, ``tiles_per_group``.  Raises NativeError above SG_MSG_MAX_LEN."""
    p = N.SgMsgPlan()
    rc = N.load().sg_msg_plan_for(n, adlen, groups, C.byref(p))
    if rc != N.SG_OK:
        raise N.NativeError(rc, "sg_msg_plan_for: a length above SG_MSG_MAX_LEN")
    return {name: int(getattr(p, name)) for name, _ in N.SgMsgPlan._fields_}


def set_groups(n: int) -> int:
    """``sg_set_msg_groups``: 0 = automatic grid, negative = query; returns the previous setting."""
    return int(N.load().sg_set_msg_groups(n))


def workspace_size() -> int:
    return int(N.load().sg_msg_workspace_size())


def _msg(key, nonce: bytes, ad, inp, in_len, out, status, keep_failed, stream, workspace) -> N.SgMsg:
    nonce = bytes(nonce)
    if len(nonce) != N.SG_NONCE_LEN:
        raise ValueError(f"nonce must be {N.SG_NONCE_LEN} bytes, got {len(nonce)}")  # chacha20.rs:27
    m = N.SgMsg()
    m.key = _ptr(key)
    m.nonce[:] = nonce
    m.ad = _ptr(ad)
    m.ad_len = int(ad.numel()) if ad is not None else 0
    m.in_ = _ptr(inp)
    m.in_len = int(inp.numel()) if in_len is None else in_len
    m.out = _ptr(out)
    m.status = _ptr(status)
    m.flags = N.SG_MSG_KEEP_FAILED if keep_failed else 0
    m.stream = _stream_handle(stream)
    m.workspace = _ptr(workspace)
    m.workspace_size = int(workspace.numel()) if workspace is not None else 0
    return m


def seal_msg(key, nonce: bytes, inp, out, ad=None, in_len=None, stream=None, workspace=None) -> None:
    """out[0, n + 16) = ct || tag of the n = ``in_len`` (default: all of ``inp``)
    bytes of ``inp`` (chacha20_poly1305.rs:48-59).  ``out`` may be ``inp`` itself."""
    m = _msg(key, nonce, ad, inp, in_len, out, None, False, stream, workspace)
    N.check(N.load().sg_seal_msg_dev(C.byref(m)))


def open_(key, nonce: bytes, inp, out, status, ad=None, in_len=None, keep_failed=False, stream=None,
          workspace=None) -> int:
    """Open ct || tag (``in_len`` bytes of ``inp``); the MAC result lands in the
    device byte ``status`` (0 ok, 1 BadRecordMac "wrong mac"), and the output of a
    failed open is zeroed on the device unless ``keep_failed``.  Returns SG_OK, or
    SG_E_SHORT for fewer than 16 bytes (nothing is touched then)."""
    if status is None:
        raise ValueError("open needs a status tensor")
    m = _msg(key, nonce, ad, inp, in_len, out, status, keep_failed, stream, workspace)
    return N.check(N.load().sg_open_msg_dev(C.byref(m)))
