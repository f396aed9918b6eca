"""TLS 1.2 key schedule (suruga src/cipher/prf.rs, src/client.rs:130-225) over
the C ABI: ``hmac_sha256``, ``Prf`` and the per-connection key derivation that
fills the key tables of the batch calls.  Host code (sg_keysched.cpp); no GPU
needed, no Python fallback.

TLS 1.3 (RFC 8446 section 7.1 - 7.3) further below: ``hkdf_extract``,
``hkdf_expand_label`` and ``tls13_traffic_keys`` on the host, and
``tls13_traffic_keys_dev``, which derives (and with ``update`` ratchets) the rows
of device tables in one launch (sg_hkdf.hip).  ``quic_packet_keys`` at the end:
the packet protection keys of RFC 9001 section 5.1 and 6.1, on the host."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


def sha256(msg: bytes) -> bytes:  # crypto/sha2.rs:18
    out = (C.c_uint8 * 32)()
    N.load().sg_sha256(msg, len(msg), out)
    return bytes(out)


def hmac_sha256(key: bytes, msg: bytes) -> bytes:  # prf.rs:8-29
    out = (C.c_uint8 * 32)()
    N.check(N.load().sg_hmac_sha256(key, len(key), msg, len(msg), out))
    return bytes(out)


class Prf:
    """prf.rs:31-89: ``Prf(secret, seed).get_bytes(n)`` continues one P_SHA256 stream."""

    def __init__(self, secret: bytes, seed: bytes):
        lib = N.load()
        self._h = lib.sg_prf_new(secret, len(secret), seed, len(seed))
        if not self._h:
            raise ValueError(N.last_error())

    def get_bytes(self, size: int) -> bytes:
        out = (C.c_uint8 * max(size, 1))()
        N.check(N.load().sg_prf_get_bytes(self._h, out, size))
        return bytes(out)[:size]

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            N.load().sg_prf_free(h)


def derive_keys(pre_master, client_random, server_random, threads: int = 8, with_master: bool = False):
    """client.rs:130-163 for many connections.

    pre_master: uint8 [count, pm_len]; randoms: uint8 [count, 32].  Returns
    (client_write_keys, server_write_keys[, master_secrets]) as uint8 arrays
    [count, 32] (and [count, 48]) -- the client encrypts with the first and
    decrypts with the second; a server the other way round."""
    pm = np.ascontiguousarray(pre_master, dtype=np.uint8)
    cr = np.ascontiguousarray(client_random, dtype=np.uint8)
    sr = np.ascontiguousarray(server_random, dtype=np.uint8)
    count = pm.shape[0]
    if cr.shape != (count, 32) or sr.shape != (count, 32):
        raise ValueError("randoms must be [count, 32]")
    cw = np.empty((count, 32), dtype=np.uint8)
    sw = np.empty((count, 32), dtype=np.uint8)
    ms = np.empty((count, 48), dtype=np.uint8) if with_master else None
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    N.check(N.load().sg_derive_keys(count, p(pm), pm.shape[1], pm.shape[1], p(cr), p(sr), p(ms), p(cw), p(sw),
                                    threads))
    return (cw, sw, ms) if with_master else (cw, sw)


def derive_keys_ivs(pre_master, client_random, server_random, threads: int = 8, with_master: bool = False):
    """derive_keys with the write IVs of RFC 7905 (sg_derive_keys_ivs): returns
    (client_write_keys, server_write_keys, client_write_ivs, server_write_ivs[, master_secrets]),
    the IVs as uint8 [count, 12] -- the 88-byte key block of RFC 5246 section 6.3
    with no MAC keys; the keys are derive_keys' bytes."""
    pm = np.ascontiguousarray(pre_master, dtype=np.uint8)
    cr = np.ascontiguousarray(client_random, dtype=np.uint8)
    sr = np.ascontiguousarray(server_random, dtype=np.uint8)
    count = pm.shape[0]
    if cr.shape != (count, 32) or sr.shape != (count, 32):
        raise ValueError("randoms must be [count, 32]")
    cw = np.empty((count, 32), dtype=np.uint8)
    sw = np.empty((count, 32), dtype=np.uint8)
    ci = np.empty((count, 12), dtype=np.uint8)
    si = np.empty((count, 12), dtype=np.uint8)
    ms = np.empty((count, 48), dtype=np.uint8) if with_master else None
    p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None  # noqa: E731
    N.check(N.load().sg_derive_keys_ivs(count, p(pm), pm.shape[1], pm.shape[1], p(cr), p(sr), p(ms), p(cw), p(sw),
                                        p(ci), p(si), threads))
    return (cw, sw, ci, si, ms) if with_master else (cw, sw, ci, si)


def verify_data(master_secret: bytes, server: bool, handshake_hash: bytes) -> bytes:  # client.rs:184-221
    out = (C.c_uint8 * 12)()
    N.check(N.load().sg_finished_verify_data(master_secret, int(server), handshake_hash, out))
    return bytes(out)


# ---- TLS 1.3 (RFC 8446 section 7.1 - 7.3): HKDF with SHA-256, traffic keys, KeyUpdate ----
def hkdf_extract(salt: bytes, ikm: bytes) -> bytes:
    """RFC 5869 section 2.2 (``sg_hkdf_extract``); an empty or None salt is 32 zero bytes."""
    salt = bytes(salt or b"")
    out = (C.c_uint8 * 32)()
    N.check(N.load().sg_hkdf_extract(salt or None, len(salt), bytes(ikm) or None, len(ikm), out))
    return bytes(out)


def hkdf_expand_label(secret: bytes, label: bytes, context: bytes, length: int) -> bytes:
    """RFC 8446 section 7.1 (``sg_hkdf_expand_label``): ``label`` without the "tls13 " prefix."""
    secret, label, context = bytes(secret), bytes(label), bytes(context)
    if len(secret) != 32:
        raise ValueError("the secret must be 32 bytes (SHA-256)")
    out = (C.c_uint8 * max(length, 1))()
    N.check(N.load().sg_hkdf_expand_label(secret, label or None, len(label), context or None, len(context), out,
                                          length))
    return bytes(out)[:length]


def tls13_traffic_keys(secrets, update: bool = False, threads: int = 8):
    """RFC 8446 section 7.3 for many connections (``sg_tls13_traffic_keys``).

    secrets: uint8 [count, 32], the traffic secrets.  Returns (keys, ivs) as uint8
    arrays [count, 32] and [count, 12], the tables of the TLS 1.3 batch calls.
    With ``update`` every secret takes one KeyUpdate step first (section 7.2) and
    the call returns (keys, ivs, next_secrets); the argument is left as it was."""
    sec = np.array(secrets, dtype=np.uint8, order="C")  # a copy: the C call ratchets in place
    if sec.ndim != 2 or sec.shape[1] != 32:
        raise ValueError("secrets must be [count, 32]")
    count = sec.shape[0]
    keys = np.empty((count, 32), dtype=np.uint8)
    ivs = np.empty((count, 12), dtype=np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N.check(N.load().sg_tls13_traffic_keys(count, p(sec), p(keys), p(ivs), int(bool(update)), threads))
    return (keys, ivs, sec) if update else (keys, ivs)


def tls13_traffic_keys_dev(secrets, keys=None, ivs=None, index=None, update: bool = False, stream=None) -> None:
    """The same over device tensors in one launch (``sg_tls13_traffic_keys_dev``).

    secrets: uint8 [rows, 32] on the device; keys [rows, 32] and ivs [rows, 12] (either may
    be None) receive the rows' keys and write IVs; index: uint32 [count] row numbers, or
    None for every row.  With ``update`` the selected secrets are ratcheted in place first.
    Ordered on ``stream`` (None: torch's current stream) like a batch call."""
    from .batch import _ptr, _stream_handle

    k = N.SgTls13Keys()
    k.rows = int(secrets.numel()) // 32
    k.count = int(index.numel()) if index is not None else k.rows
    k.flags = N.SG_TLS13_KEYS_UPDATE if update else 0
    k.index, k.secrets, k.keys, k.ivs = _ptr(index), _ptr(secrets), _ptr(keys), _ptr(ivs)
    k.stream = _stream_handle(stream)
    N.check(N.load().sg_tls13_traffic_keys_dev(C.byref(k)))


def quic_packet_keys(secrets, update: bool = False, threads: int = 8):
    """RFC 9001 section 5.1 for many connections (``sg_quic_packet_keys``).

    secrets: uint8 [count, 32], the packet protection secrets.  Returns (keys, ivs, hps) as
    uint8 arrays [count, 32], [count, 12] and [count, 32], the tables of ``quic.QuicBatch``.
    With ``update`` every secret takes one key update step first ("quic ku", section 6.1) and
    the call returns (keys, ivs, next_secrets): the header protection keys do not change at
    a key update.  The argument is left as it was."""
    sec = np.array(secrets, dtype=np.uint8, order="C")  # a copy: the C call ratchets in place
    if sec.ndim != 2 or sec.shape[1] != 32:
        raise ValueError("secrets must be [count, 32]")
    count = sec.shape[0]
    keys = np.empty((count, 32), dtype=np.uint8)
    ivs = np.empty((count, 12), dtype=np.uint8)
    hps = None if update else np.empty((count, 32), dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)  # noqa: E731
    N.check(N.load().sg_quic_packet_keys(count, p(sec), p(keys), p(ivs), p(hps), int(bool(update)), threads))
    return (keys, ivs, sec) if update else (keys, ivs, hps)
