"""What the QUIC packet protection tests share -- TEST INFRASTRUCTURE ONLY.

* ``Pkt`` / ``QuicCase``: a batch on the host -- every packet's first byte, packet number
  offset, packet number, payload, connection and where it lies -- with the reference's
  (tests/quic_ref.py) protected packets, computed once.
* whole-buffer runs: every device buffer starts as footprint.sentinel with a margin in
  front and behind and the *whole* buffer, the status bytes and pn_out are compared
  afterwards, so a stray write fails as a wrong byte does.
* ``forge_lanes``: ciphertext under which every per-lane sum of the kernel's MAC
  (tests/quic_model.py) has a chosen value.

Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

import footprint as fp
import quic_model as QM
import quic_ref as Q
import rfc8439_ref as R

M = fp.MARGIN
P = QM.P
KEYS3 = R.KEYS
IVS3 = b"".join(hashlib.sha256(b"quic iv %d" % i).digest()[:12] for i in range(3))
HPS3 = b"".join(hashlib.sha256(b"quic hp %d" % i).digest() for i in range(3))
PN_EDGES = (0, 2**32 - 1, 2**32, 2**62 - 1)
PN_OFFS = (1, 9, 21, 251)
JUNK = 0xAA  # what the input's packet number field holds: the seal ignores it


def rnd(n: int, what: str) -> bytes:
    return R.data(n, what.encode())


@dataclass
class Pkt:
    b0: int            # unprotected first byte
    pn_off: int
    pn: int
    payload: bytes
    kidx: int = 0
    exp: int = None    # open: the expected packet number (default: pn itself)
    tag: str = ""

    @property
    def pn_len(self):
        return (self.b0 & 3) + 1

    @property
    def hdr_len(self):
        return self.pn_off + self.pn_len

    def raw(self) -> bytes:
        """header || payload as a seal takes it, the packet number field full of JUNK."""
        return bytes([self.b0]) + rnd(self.pn_off - 1, f"hdr {self.tag} {self.pn_off}") + bytes([JUNK]) * self.pn_len + self.payload

    def header(self) -> bytes:
        return Q.header_of(self.raw(), self.pn_off, self.pn)


def short(pn_len: int, phase: int = 0) -> int:
    return 0x40 | (phase << 2) | (pn_len - 1)


def long_(pn_len: int) -> int:
    return 0xC0 | (pn_len - 1)


def offsets(lens, skew):
    """Packets one behind the other, each at a multiple of 16 plus skew(i)."""
    off, pos = [], 0
    for i, n in enumerate(lens):
        pos = fp.round_up(pos, 16) + skew(i)
        off.append(pos)
        pos += int(n)
    return np.array(off, dtype=np.uint64), fp.round_up(pos, 16)


class QuicCase:
    """Packets with tables of `rows` connections (key_phase: two generations each, rows 2 k + phase)."""

    def __init__(self, pkts, keys=KEYS3, ivs=IVS3, hps=HPS3, key_phase=False, in_skew=lambda i: i % 16,
                 out_skew=lambda i: (i // 16 + 5 * i) % 16, strides=None):
        """The packets lie one behind the other at a multiple of 16 plus the skews -- every pair
        of skews within 256 packets -- or, with strides = (raw stride, raw base, protected
        stride, protected base), at equal distances, as the uniform fields need them."""
        self.pkts, self.keys, self.ivs, self.hps, self.key_phase = list(pkts), keys, ivs, hps, key_phase
        self.count = len(self.pkts)
        self.num_keys = len(keys) // 32
        self.rows = self.num_keys // 2 if key_phase else self.num_keys
        assert len(ivs) == 12 * self.num_keys and len(hps) == 32 * self.rows
        self.raw_lens = np.array([len(p.raw()) for p in self.pkts], dtype=np.uint32)
        if strides is None:
            self.raw_off, self.raw_size = offsets(self.raw_lens, in_skew)
            self.prot_off, self.prot_size = offsets(self.raw_lens + 16, out_skew)
        else:
            si, bi, so, bo = strides
            assert si >= int(self.raw_lens.max()) and so >= int(self.raw_lens.max()) + 16
            self.raw_off = np.arange(self.count, dtype=np.uint64) * np.uint64(si) + np.uint64(bi)
            self.prot_off = np.arange(self.count, dtype=np.uint64) * np.uint64(so) + np.uint64(bo)
            self.raw_size, self.prot_size = fp.round_up(bi + si * self.count, 16), fp.round_up(bo + so * self.count, 16)
        self._protected = {}

    def conn(self, i) -> int:
        return min(self.pkts[i].kidx, self.rows - 1)

    def tables(self, i):
        """((key, iv) per phase, hp) of packet i's connection."""
        c = self.conn(i)
        rows = (2 * c, 2 * c + 1) if self.key_phase else (c, c)
        return ([self.keys[32 * r:32 * r + 32] for r in rows], [self.ivs[12 * r:12 * r + 12] for r in rows],
                self.hps[32 * c:32 * c + 32])

    def protected(self, i):
        """The reference's protected packet i (None: no full sample), computed once."""
        if i not in self._protected:
            p = self.pkts[i]
            keys, ivs, hp = self.tables(i)
            phase = 0 if p.b0 & 0x80 else (p.b0 >> 2) & 1
            self._protected[i] = Q.protect(keys[phase], ivs[phase], hp, p.pn, p.raw(), p.pn_off)
        return self._protected[i]

    def opened(self, i, pkt: bytes):
        """(rc, header || plaintext, pn) of `pkt` in packet i's place, as the reference opens it."""
        p = self.pkts[i]
        keys, ivs, hp = self.tables(i)
        return Q.unprotect(keys, ivs, hp, p.pn if p.exp is None else p.exp, pkt, p.pn_off)

    # ---- device arguments
    def common(self, uniform=False) -> dict:
        from gpu_support import dev_bytes, dev_u32

        c = dict(count=self.count, keys=dev_bytes(self.keys), ivs=dev_bytes(self.ivs), hp_keys=dev_bytes(self.hps),
                 key_phase=self.key_phase)
        if uniform:
            assert len({p.pn_off for p in self.pkts}) == 1 and all(p.kidx == 0 for p in self.pkts)
            c["uniform_pn_off"] = self.pkts[0].pn_off
        else:
            c.update(key_index=dev_u32([p.kidx for p in self.pkts]), pn_off=dev_u32([p.pn_off for p in self.pkts]))
        return c


def _layout_args(lens, in_off, out_off, uniform, max_len):
    from gpu_support import dev_u32, dev_u64

    if uniform:
        si, so = int(in_off[1] - in_off[0]), int(out_off[1] - out_off[0])
        assert len(set(lens.tolist())) == 1 and all(int(o) == int(in_off[0]) + si * i for i, o in enumerate(in_off))
        assert all(int(o) == int(out_off[0]) + so * i for i, o in enumerate(out_off))
        return dict(uniform_len=int(lens[0]), in_stride=si, out_stride=so), int(in_off[0]), int(out_off[0])
    return dict(lens=dev_u32(lens), max_len=int(lens.max()) if max_len is None else max_len, in_off=dev_u64(in_off),
                out_off=dev_u64(out_off)), 0, 0


def seal_whole(case: QuicCase, *, uniform=False, max_len=None, exp_st=None, where=(), stream=None):
    """Seal into a sentinel buffer with margins: the whole output is the sentinel with every
    protected packet of the reference laid over it (nothing for a status 2 or 3), the input
    is unchanged, the statuses are exp_st (default: 0 for every packet the reference protects,
    2 for the others) and pn_out, which a seal does not read, is untouched."""
    from suruga_amd import quic as QU

    if exp_st is None:
        exp_st = [0 if case.protected(i) is not None else 2 for i in range(case.count)]
    in_img = fp.image(M + case.raw_size + M, 0x31, [(M + int(o), p.raw()) for o, p in zip(case.raw_off, case.pkts)])
    out_size = M + case.prot_size + M
    want = fp.image(out_size, 0x5A, [(M + int(case.prot_off[i]), case.protected(i)) for i in range(case.count)
                                     if exp_st[i] == 0])
    rs = [(M + int(o), M + int(o) + int(n) + 16) for o, n in zip(case.prot_off, case.raw_lens)]
    lay, bi, bo = _layout_args(case.raw_lens, case.raw_off, case.prot_off, uniform, max_len)
    from gpu_support import dev_u64

    pn = dev_u64([p.pn for p in case.pkts])
    o = fp.run_whole(lambda d: QU.seal_quic(QU.QuicBatch(inp=d["inp"][M + bi:], out=d["out"][M + bo:], status=d["status"],
                                                         pn=pn, pn_out=d["pn_out"], stream=stream,
                                                         **case.common(uniform), **lay)),
                     in_img, fp.sentinel(out_size, 0x5A), want, rs,
                     arrays={"status": fp.array_start(case.count, 0x51), "pn_out": fp.array_start(case.count, 0x52, np.uint64)})
    o.check(exp_st, None, where=(*where, "seal"))
    return o


def open_whole(case: QuicCase, pkts=None, *, lens=None, keep=False, uniform=False, max_len=None, exp=None, where=()):
    """Open pkts (default: the reference's protected packets), laid out like the seal's output,
    into a sentinel buffer.  exp[i] = (status, bytes or None, pn_out or None) replaces what the
    reference says of packet i: per packet the whole output is header || plaintext (status 0),
    len - 16 zero bytes and pn_out 0 (status 1), the decryption and its number (status 1 with
    keep) or nothing, pn_out included (status 2, 3)."""
    from gpu_support import dev_u64
    from suruga_amd import quic as QU

    pkts = [case.protected(i) for i in range(case.count)] if pkts is None else pkts
    lens = np.array([len(p) for p in pkts], dtype=np.uint32) if lens is None else np.asarray(lens, dtype=np.uint32)
    in_img = fp.image(M + case.prot_size + M, 0x33, [(M + int(o), p) for o, p in zip(case.prot_off, pkts)])
    out_size = M + case.raw_size + M
    parts, st, pn_out = [], [], {}
    for i in range(case.count):
        if exp is not None and i in exp:
            rc, body, pn = exp[i]
        else:
            rc, body, pn = case.opened(i, pkts[i][:int(lens[i])])
            if rc == 1 and not keep:
                body, pn = bytes(len(body)), 0
            elif rc == 2:
                body, pn = None, None
        st.append(rc)
        if body is not None:
            parts.append((M + int(case.raw_off[i]), body))
        if pn is not None:
            pn_out[i] = pn
    start_pn = fp.array_start(case.count, 0x52, np.uint64)
    want_pn = start_pn.copy()
    for i, v in pn_out.items():
        want_pn[i] = v
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.raw_off, case.raw_lens)]
    lay, bi, bo = _layout_args(lens, case.prot_off, case.raw_off, uniform, max_len)
    pn = dev_u64([p.pn if p.exp is None else p.exp for p in case.pkts])
    o = fp.run_whole(lambda d: QU.open_quic(QU.QuicBatch(inp=d["inp"][M + bi:], out=d["out"][M + bo:], status=d["status"],
                                                         pn=pn, pn_out=d["pn_out"], keep_failed=keep,
                                                         **case.common(uniform), **lay)),
                     in_img, fp.sentinel(out_size, 0xA5), fp.image(out_size, 0xA5, parts), rs,
                     arrays={"status": fp.array_start(case.count, 0x51), "pn_out": start_pn})
    o.check(st, want_pn[:case.count].tolist(), where=(*where, "open"))
    return o


# ---------------------------------------------------------------------------
# forged per-lane sums
# ---------------------------------------------------------------------------
def forge_lanes(key: bytes, nonce12: bytes, ad: bytes, n: int, G: int, target: int, seed: str):
    """(ct, tries, skipped): n ciphertext bytes under which every lane sum H_t and slot 0's TS of the
    kernel's MAC (quic_model.lane_sets) is == target (mod p).  Per set, one whole ciphertext
    block is solved for -- c = (target - rest) r^-(E - b), a block value when c - 2^128 lies in
    [0, 2^128), about one try in four -- and the set's other ciphertext blocks are drawn again
    until it is.  A set without a whole ciphertext block (a lane that holds the additional
    data alone) cannot be steered and is left as it falls: `skipped` counts those."""
    r16, _ = R.poly_key(key, nonce12)
    r = int.from_bytes(r16, "little") & R.CLAMP
    na = (len(ad) + 15) // 16
    ct = bytearray(rnd(n, f"lanes {seed}"))
    tries = skipped = 0
    for t, blocks in QM.lane_sets(len(ad), n, G):
        whole = [b for b in blocks if b >= na and 16 * (b - na) + 16 <= n]
        if not whole:
            skipped += 1
            continue
        free, E = whole[-1], blocks[-1] + 1
        inv = pow(pow(r, E - free, P), -1, P)
        for k in range(200):
            stream = R.mac_stream(ad, bytes(ct))
            rest = sum((int.from_bytes(stream[16 * i:16 * i + 16], "little") + (1 << 128)) * pow(r, E - i, P)
                       for i in blocks if i != free) % P
            c = (target - rest) * inv % P
            tries += 1
            if (1 << 128) <= c < (1 << 129):
                ct[16 * (free - na):16 * (free - na) + 16] = (c - (1 << 128)).to_bytes(16, "little")
                break
            other = [b for b in whole if b != free]
            assert other, "one whole ciphertext block and nothing to draw again"
            b = other[k % len(other)]
            ct[16 * (b - na):16 * (b - na) + 16] = rnd(16, f"lanes {seed} {t} {k}")
        else:
            raise AssertionError("no forgery in 200 tries")
    return bytes(ct), tries, skipped
