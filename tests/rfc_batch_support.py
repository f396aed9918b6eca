"""What the RFC 8439 record-batch tests share -- TEST INFRASTRUCTURE ONLY.

* ``RfcCase``: gpu_support.BatchCase with 12-byte nonces and, in TLS mode, the
  write IVs of RFC 7905 (nonce = iv[key] XOR (00 00 00 00 || be64(seq))).
* ``REF``: tests/rfc8439_ref.py in the shape gpu_support.check_sealed expects of a
  reference (``seal``, ``tls_ad``), plus ``open``.
* whole-buffer runs: every device buffer starts as footprint.sentinel with a
  margin in front and behind, and the *whole* buffer is compared afterwards, so a
  stray write fails as a wrong byte does.
* a forger for the RFC stream, in which every block is full: fix every block but
  one ciphertext block, solve for it, reseed until it is below 2^128.

Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
import struct

import numpy as np

import footprint as fp
import rfc8439_ref as R
from gpu_support import BatchCase, dev_bytes, slots

P = (1 << 130) - 5
M = fp.MARGIN
KEYS3 = R.KEYS  # three keys
IVS3 = hashlib.sha256(b"rfc7905 iv 0").digest()[:12] + b"\xff" * 12 + hashlib.sha256(b"rfc7905 iv 2").digest()[:12]
SEQ_EDGES = (0, 1, 2**32 - 1, 2**32, 2**64 - 1, 2**63, 0x0102030405060708, 2**32 + 1)


def tls_nonce(iv12: bytes, seq: int) -> bytes:
    """RFC 7905 section 2: the 12-byte write IV XOR the sequence number, left-padded to 12."""
    pad = bytes(4) + struct.pack(">Q", seq)
    return bytes(a ^ b for a, b in zip(iv12, pad))


def tls_ad(seq: int, n: int, content_type: int = 23, major: int = 3, minor: int = 3) -> bytes:
    """RFC 5246 section 6.2.3.3: seq || type || version || length, 13 bytes."""
    return struct.pack(">QBBBH", seq, content_type, major, minor, n)


class Ref:
    """rfc8439_ref as check_sealed's `oracle`."""

    seal = staticmethod(R.seal)
    open = staticmethod(R.open)
    tls_ad = staticmethod(tls_ad)


REF = Ref()


class RfcCase(BatchCase):
    """BatchCase through sg_*_batch_rfc8439: nonces_h holds 12 bytes per record;
    ivs_h (TLS mode) 12 bytes per key."""

    def __init__(self, *args, ivs_h=None, **kw):
        super().__init__(*args, **kw)
        self.ivs_h = ivs_h
        self._expected = {}
        assert (ivs_h is not None and len(ivs_h) == 12 * self.num_keys) if self.tls else ivs_h is None

    def key_slot(self, i) -> int:
        k = 0 if self.kidx is None else int(self.kidx[i])
        return min(k, self.num_keys - 1) if self.clamp_keys else k

    def nonce_ad(self, oracle, i):
        if self.tls:
            header = () if self.content_type is None else (self.content_type, *self.version)
            k = self.key_slot(i)
            return tls_nonce(self.ivs_h[12 * k:12 * k + 12], self.seq(i)), oracle.tls_ad(self.seq(i), self.n(i), *header)
        a = i * self.ad_stride
        return bytes(self.nonces_h[12 * i:12 * i + 12]), bytes(self.ads_h[a:a + self.adlen])

    def expected(self, oracle, i) -> bytes:
        """The reference's ct || tag of record i, computed once."""
        if i not in self._expected:
            self._expected[i] = super().expected(oracle, i)
        return self._expected[i]

    def common(self, ads_h=None) -> dict:
        c = super().common(ads_h)
        c["rfc8439"] = True
        if self.tls:
            c["ivs"] = dev_bytes(self.ivs_h).view(self.num_keys, 12)
        return c

    def open_args(self, olens=None, max_len=None, ads_h=None, ivs_h=None) -> dict:
        """BatchCase.open_args; ivs_h: other write IVs for this call."""
        args = super().open_args(olens, max_len, ads_h)
        return args if ivs_h is None else dict(args, ivs=dev_bytes(ivs_h).view(self.num_keys, 12))

    def decrypted(self, i, data: bytes) -> bytes:
        """The always-computed decryption of `data` (ct || tag) under record i's key and nonce."""
        nonce, _ = self.nonce_ad(REF, i)
        return R.xor_stream(self.key(i), nonce, data[:-16])


def rnd(n: int, what: str) -> bytes:
    return R.data(n, what.encode())


def poly_rs(key: bytes, nonce12: bytes):
    """The Poly1305 key of a record as integers: r clamped, and s."""
    r16, s16 = R.poly_key(key, nonce12)
    return int.from_bytes(r16, "little") & R.CLAMP, int.from_bytes(s16, "little")


def model_record(kslot: int, seq: int, iv12: bytes | None = None):
    """(key, nonce, r, s) of a TLS record under key slot kslot, for the CPU models of the
    kernels' MACs: the slot's key and write IV (or iv12), the nonce rule above, which is
    TLS 1.3's too."""
    key = KEYS3[32 * kslot:32 * kslot + 32]
    nonce = tls_nonce(IVS3[12 * kslot:12 * kslot + 12] if iv12 is None else iv12, seq)
    return (key, nonce) + poly_rs(key, nonce)


def listed_case(lens, *, mode, skew=(0, 0), align=16, kidx=None, keys=KEYS3, tag="", **kw) -> RfcCase:
    """A listed batch of `lens` (mode "tls" or an explicit AD length): records in slots
    of `align` plus skew bytes, plaintext and, in explicit mode, nonces and ADs from SHAKE."""
    lens = np.asarray(lens)
    in_off, out_off, pt_bytes, _ = slots(lens, align, skew)
    pt = bytearray(fp.sentinel(max(pt_bytes, 1), 0x77).tobytes())
    for i, n in enumerate(lens):
        pt[int(in_off[i]):int(in_off[i]) + int(n)] = rnd(int(n), f"{tag} pt {i} {n}")
    if mode == "tls":
        return RfcCase(lens, bytes(pt), keys, in_off=in_off, out_off=out_off, kidx=kidx, **kw)
    stride = max(mode, 1)
    nonces = b"".join(rnd(12, f"{tag} nonce {i}") for i in range(len(lens)))
    ads = b"".join(rnd(mode, f"{tag} ad {i}").ljust(stride, b"\0") for i in range(len(lens)))
    return RfcCase(lens, bytes(pt), keys, in_off=in_off, out_off=out_off, kidx=kidx, nonces_h=nonces, ads_h=ads,
                   adlen=mode, **kw)


def uniform_case(n, count, *, mode, strides=None, kidx=None, keys=KEYS3, tag="", pts=None, nonces=None, ads=None,
                 **kw) -> RfcCase:
    """A uniform strided batch (16-byte aligned strides unless given); pts, nonces and
    ads (a list of per-record ADs) replace the SHAKE-derived ones."""
    si, so = strides or (fp.round_up(n, 16), fp.round_up(n + 16, 16))
    pt = bytearray(fp.sentinel(max(si * count, 1), 0x77).tobytes())
    for i in range(count):
        pt[si * i:si * i + n] = rnd(n, f"{tag} upt {i} {n}") if pts is None else pts[i]
    lens = np.full(count, n)
    if mode == "tls":
        return RfcCase(lens, bytes(pt), keys, strides=(si, so), kidx=kidx, **kw)
    stride = max(mode, 1)
    if nonces is None:
        nonces = b"".join(rnd(12, f"{tag} unonce {i}") for i in range(count))
    if ads is None:
        ads = [rnd(mode, f"{tag} uad {i}") for i in range(count)]
    ads = b"".join(a.ljust(stride, b"\0") for a in ads)
    return RfcCase(lens, bytes(pt), keys, strides=(si, so), kidx=kidx, nonces_h=nonces, ads_h=ads, adlen=mode, **kw)


# ---------------------------------------------------------------------------
# whole-buffer runs
# ---------------------------------------------------------------------------
def _extent(off, lens) -> int:
    return int(max(int(o) + int(n) for o, n in zip(off, lens))) if len(lens) else 0


def seal_whole(case: RfcCase, *, where=(), **extra) -> bytes:
    """Seal into a sentinel buffer with margins; the whole output buffer must be the
    sentinel with every record's reference ct || tag laid over it and the input
    unchanged.  Returns the sealed bytes from the first record's base on."""
    from suruga_amd import batch as B

    out_size = M + fp.round_up(_extent(case.out_off, case.lens.astype(np.int64) + 16), 16) + M
    in_img = np.concatenate([fp.sentinel(M, 0x31), np.frombuffer(case.pt_h, dtype=np.uint8), fp.sentinel(M, 0x32)])
    want = fp.image(out_size, 0x5A, [(M + int(case.out_off[i]), case.expected(REF, i)) for i in range(case.count)])
    rs = [(M + lo, M + hi) for lo, hi in (case.out_range(i) for i in range(case.count))]
    o = fp.run_whole(lambda d: B.seal(B.Batch(inp=d["inp"][M:], out=d["out"][M:], **case.seal_args(), **extra)),
                     in_img, fp.sentinel(out_size, 0x5A), want, rs)
    o.check(where=(*where, "seal"))
    return o.out[M:out_size - M].tobytes()


def open_whole(case: RfcCase, sealed: bytes, exp_st, *, keep=False, olens=None, where=(), ads_h=None, ivs_h=None,
               **extra):
    """Open `sealed` (laid out as seal_whole returned it) into a sentinel buffer: the
    whole output is the sentinel with, per record, the plaintext (status 0), exactly n
    zero bytes (status 1), the decryption (status 1 with keep) or nothing (status 2);
    the statuses are exp_st and the bytes behind them untouched."""
    from suruga_amd import batch as B

    exp_st = bytes(exp_st)
    out_size = M + fp.round_up(_extent(case.in_off, case.lens), 16) + M
    in_img = np.concatenate([fp.sentinel(M, 0x33), np.frombuffer(bytes(sealed), dtype=np.uint8), fp.sentinel(M, 0x34)])
    parts = []
    for i in range(case.count):
        lo, hi = case.out_range(i)
        if exp_st[i] == 0:
            parts.append((M + int(case.in_off[i]), case.pt(i)))
        elif exp_st[i] == 1:
            parts.append((M + int(case.in_off[i]), case.decrypted(i, sealed[lo:hi]) if keep else bytes(case.n(i))))
    args = case.open_args(olens, ads_h=ads_h, ivs_h=ivs_h)
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.in_off, case.lens)]
    o = fp.run_whole(lambda d: B.open_(B.Batch(inp=d["inp"][M:], out=d["out"][M:], status=d["status"], keep_failed=keep,
                                               **args, **extra)),
                     in_img, fp.sentinel(out_size, 0xA5), fp.image(out_size, 0xA5, parts), rs,
                     arrays={"status": fp.array_start(case.count, 0x51)})
    o.check(exp_st, where=(*where, "open"))


# ---------------------------------------------------------------------------
# forged accumulators
# ---------------------------------------------------------------------------
ACC_TARGETS = {"0": 0, "p-1": P - 1, "p": P, "p+4": P + 4, "2^130-1": 2**130 - 1}


def forge_ct(key: bytes, nonce12: bytes, ad: bytes, n: int, target: int, seed: str):
    """(ct, tries): n ciphertext bytes (n a multiple of 16, n >= 32) whose Poly1305
    accumulator over the RFC stream is == target (mod p) before s is added.  Every block
    of the stream is full, so with all blocks but ciphertext block 0 fixed the missing
    one is (target - rest) r^-(B - j) - 2^128, usable when it lies in [0, 2^128):
    about one try in four; the other blocks are redrawn until it does."""
    assert n % 16 == 0 and n >= 32
    r16, _ = R.poly_key(key, nonce12)
    r = int.from_bytes(r16, "little") & R.CLAMP
    beta = -(-len(ad) // 16)
    for t in range(200):
        ct = bytearray(rnd(n, f"forge {seed} {t}"))
        ct[:16] = bytes(16)
        stream = R.mac_stream(ad, bytes(ct))
        B = len(stream) // 16
        h = 0
        for j in range(B):
            h = (h + int.from_bytes(stream[16 * j:16 * j + 16], "little") + (1 << 128)) * r % P
        # block beta (the first ciphertext block) has weight r^(B - beta); it is 2^128 + 0 so far
        w = pow(r, B - beta, P)
        c = (target - h) * pow(w, -1, P) % P
        if c < (1 << 128):
            ct[:16] = c.to_bytes(16, "little")
            return bytes(ct), t + 1
    raise AssertionError("no forgery in 200 tries")


def accumulator(key: bytes, nonce12: bytes, ad: bytes, ct: bytes) -> int:
    r16, _ = R.poly_key(key, nonce12)
    r = int.from_bytes(r16, "little") & R.CLAMP
    stream = R.mac_stream(ad, ct)
    h = 0
    for j in range(len(stream) // 16):
        h = (h + int.from_bytes(stream[16 * j:16 * j + 16], "little") + (1 << 128)) * r % P
    return h
