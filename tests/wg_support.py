"""What the WireGuard transport data tests share -- TEST INFRASTRUCTURE ONLY.

* ``Pkt`` / ``WgCase``: a batch on the host -- every inner packet, its counter, its session
  and where it lies -- with the reference's (tests/wg_ref.py) messages, computed once.
* whole-buffer runs: every device buffer starts as footprint.sentinel with a margin in
  front and behind and the *whole* buffer, the status bytes, counter_out and inner_len are
  compared afterwards, so a stray write, an unwritten padding byte or a counter_out that a
  seal touched fails as a wrong byte does.  In place (``inplace=True``) there is one
  buffer: message i at its offset, its inner packet 16 bytes behind that.

Imports without torch and without a GPU."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import footprint as fp
import rfc8439_ref as R
import wg_ref as W
from quic_support import offsets

M = fp.MARGIN
KEYS3 = R.KEYS
RECEIVERS3 = (0x01020304, 0xFFFFFFFF, 0x80000001)
COUNTER_EDGES = (0, 2**32 - 1, 2**32, 2**64 - 2**13 - 2)


def rnd(n: int, what: str) -> bytes:
    return R.data(n, what.encode())


@dataclass
class Pkt:
    inner: bytes
    counter: int
    kidx: int = 0


def inner_packet(n: int, i: int) -> bytes:
    """n bytes: an IPv4 packet of n bytes, an IPv6 one for every third that has room, any bytes below 20."""
    if n >= 40 and i % 3 == 1:
        return W.ipv6(n - 40, n, f"p{i}")
    return W.ipv4(n, n, f"p{i}") if n >= 20 else rnd(n, f"short inner {n} {i}")


class WgCase:
    """Inner packets with a table of sessions.  A packet's plaintext slot holds its padded
    length, a message's slot 32 bytes more."""

    def __init__(self, pkts, keys=KEYS3, receivers=RECEIVERS3, pad_cap=0, in_skew=lambda i: i % 16,
                 out_skew=lambda i: (i // 16 + 5 * i) % 16, strides=None, inplace=False):
        """The packets lie one behind the other at a multiple of 16 plus the skews -- every pair
        of skews within 256 packets -- or, with strides = (inner stride, inner base, message
        stride, message base), at equal distances, as the uniform fields need them."""
        self.pkts, self.keys, self.receivers, self.pad_cap, self.inplace = list(pkts), keys, tuple(receivers), pad_cap, inplace
        self.count = len(self.pkts)
        self.num_keys = len(keys) // 32
        assert len(self.receivers) == self.num_keys
        self.lens = np.array([len(p.inner) for p in self.pkts], dtype=np.uint32)
        self.padded = np.array([W.padded_len(len(p.inner), pad_cap) for p in self.pkts], dtype=np.uint32)
        self.msg_lens = self.padded + np.uint32(32)
        if strides is None:
            self.msg_off, self.msg_size = offsets(self.msg_lens, out_skew)
            self.raw_off, self.raw_size = offsets(self.padded, in_skew)
        else:
            si, bi, so, bo = strides
            assert si >= int(self.padded.max()) and so >= int(self.msg_lens.max())
            self.raw_off = np.arange(self.count, dtype=np.uint64) * np.uint64(si) + np.uint64(bi)
            self.msg_off = np.arange(self.count, dtype=np.uint64) * np.uint64(so) + np.uint64(bo)
            self.raw_size, self.msg_size = fp.round_up(bi + si * self.count, 16), fp.round_up(bo + so * self.count, 16)
        if inplace:
            self.raw_off, self.raw_size = self.msg_off + np.uint64(16), self.msg_size
        self._protected = {}

    def row(self, i) -> int:
        return min(self.pkts[i].kidx, self.num_keys - 1)

    def key(self, i) -> bytes:
        return self.keys[32 * self.row(i):32 * self.row(i) + 32]

    def protected(self, i) -> bytes:
        """The reference's message i, computed once."""
        if i not in self._protected:
            p = self.pkts[i]
            self._protected[i] = W.protect(self.key(i), self.receivers[self.row(i)], p.counter, p.inner, self.pad_cap)
        return self._protected[i]

    # ---- device arguments
    def common(self, uniform=False) -> dict:
        from gpu_support import dev_bytes, dev_u32

        c = dict(count=self.count, keys=dev_bytes(self.keys))
        if uniform:
            assert all(p.kidx == 0 for p in self.pkts)
        else:
            c["key_index"] = dev_u32([p.kidx for p in self.pkts])
        return c


def layout_args(lens, in_off, out_off, uniform, max_len):
    """The length and placement keywords of a WgBatch, and the bases the uniform form starts from."""
    from gpu_support import dev_u32, dev_u64

    if uniform:
        n = len(lens)
        si = int(in_off[1] - in_off[0]) if n > 1 else 0
        so = int(out_off[1] - out_off[0]) if n > 1 else 0
        assert len(set(lens.tolist())) == 1 and all(int(o) == int(in_off[0]) + si * i for i, o in enumerate(in_off))
        assert all(int(o) == int(out_off[0]) + so * i for i, o in enumerate(out_off))
        return dict(uniform_len=int(lens[0]), in_stride=si, out_stride=so), int(in_off[0]), int(out_off[0])
    return dict(lens=dev_u32(lens), max_len=int(lens.max()) if max_len is None else max_len, in_off=dev_u64(in_off),
                out_off=dev_u64(out_off)), 0, 0


def _arrays(count):
    return {"status": fp.array_start(count, 0x51), "counter_out": fp.array_start(count, 0x52, np.uint64),
            "inner_len": fp.array_start(count, 0x53, np.uint32)}


SPARE = 64  # in place: the `out` buffer of the harness, which the call never sees and must leave alone


def seal_whole(case: WgCase, *, uniform=False, max_len=None, exp_st=None, where=(), stream=None):
    """Seal into a sentinel buffer with margins: the whole output is the sentinel with every
    message of the reference laid over it (nothing for a status 3), the input is unchanged
    -- in place: the one buffer is that image -- the statuses are exp_st (default: all 0) and
    counter_out and inner_len, which a seal does not read, are untouched."""
    from gpu_support import dev_u32, dev_u64
    from suruga_amd import wg as WG

    exp_st = [0] * case.count if exp_st is None else exp_st
    inners = [(M + int(o), p.inner) for o, p in zip(case.raw_off, case.pkts)]
    msgs = [(M + int(case.msg_off[i]), case.protected(i)) for i in range(case.count) if exp_st[i] == 0]
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.msg_off, case.msg_lens)]
    lay, bi, bo = layout_args(case.lens, case.raw_off, case.msg_off, uniform, max_len)
    counter = dev_u64([p.counter for p in case.pkts])
    receiver = dev_u32(case.receivers)
    size = M + case.msg_size + M
    if case.inplace:
        in_img, out0, want = fp.image(size, 0x5A, inners), fp.sentinel(SPARE, 0x77), fp.sentinel(SPARE, 0x77)
        # a skipped packet keeps its inner bytes; every other slot becomes its message
        want_inp = fp.image(size, 0x5A, [x for i, x in enumerate(inners) if exp_st[i] != 0] + msgs)
        pick = lambda d: (d["inp"][M + bi:], d["inp"][M + bo:])  # noqa: E731
    else:
        in_img, out0 = fp.image(M + case.raw_size + M, 0x31, inners), fp.sentinel(size, 0x5A)
        want, want_inp = fp.image(size, 0x5A, msgs), None
        pick = lambda d: (d["inp"][M + bi:], d["out"][M + bo:])  # noqa: E731

    def call(d):
        inp, out = pick(d)
        WG.seal_wg(WG.WgBatch(inp=inp, out=out, status=d["status"], receiver=receiver, counter=counter,
                              counter_out=d["counter_out"], inner_len=d["inner_len"], pad_cap=case.pad_cap,
                              stream=stream, **case.common(uniform), **lay))

    o = fp.run_whole(call, in_img, out0, want, [] if case.inplace else rs, want_inp=want_inp,
                     in_ranges=rs if case.inplace else (), arrays=_arrays(case.count))
    o.check(exp_st, None, None, where=(*where, "seal"))
    return o


def open_whole(case: WgCase, msgs=None, *, lens=None, keep=False, uniform=False, max_len=None, want_inner=True, where=()):
    """Open msgs (default: the reference's messages), laid out like the seal's output, into a
    sentinel buffer -- in place: where they lie, 16 bytes on.  Per packet, as the reference
    (wg_ref.unprotect) says: the whole output is the padded plaintext (status 0 and 7), zeros
    and counter_out 0 (status 1), the decryption and the wire counter (status 1 with keep), or
    nothing, counter_out and inner_len included (status 2, 3, 6).  want_inner=False: inner_len
    is NULL and its array stays as it was."""
    from suruga_amd import wg as WG

    msgs = [case.protected(i) for i in range(case.count)] if msgs is None else msgs
    lens = np.array([len(m) for m in msgs], dtype=np.uint32) if lens is None else np.asarray(lens, dtype=np.uint32)
    bound = int(lens.max()) if max_len is None else max_len
    placed = [(M + int(o), m) for o, m in zip(case.msg_off, msgs)]
    arrays = _arrays(case.count)
    st, parts = [], []
    want_ctr, want_len = arrays["counter_out"].copy(), arrays["inner_len"].copy()
    for i in range(case.count):
        rc, pt, ctr, L = W.unprotect(case.key(i), msgs[i][:int(lens[i])], want_inner, bound)
        st.append(rc)
        if pt is None:
            continue
        scrub = rc == 1 and not keep
        parts.append((M + int(case.raw_off[i]), bytes(len(pt)) if scrub else pt))
        want_ctr[i] = 0 if scrub else ctr
        if want_inner:
            want_len[i] = L
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.raw_off, case.padded)]
    lay, bi, bo = layout_args(lens, case.msg_off, case.raw_off, uniform, max_len)
    size = M + case.msg_size + M
    if case.inplace:
        in_img, out0, want = fp.image(size, 0x33, placed), fp.sentinel(SPARE, 0x77), fp.sentinel(SPARE, 0x77)
        want_inp = fp.image(size, 0x33, placed + parts)
        pick = lambda d: (d["inp"][M + bi:], d["inp"][M + bo:])  # noqa: E731
    else:
        in_img, out_size = fp.image(size, 0x33, placed), M + case.raw_size + M
        out0, want, want_inp = fp.sentinel(out_size, 0xA5), fp.image(out_size, 0xA5, parts), None
        pick = lambda d: (d["inp"][M + bi:], d["out"][M + bo:])  # noqa: E731

    def call(d):
        inp, out = pick(d)
        WG.open_wg(WG.WgBatch(inp=inp, out=out, status=d["status"], counter_out=d["counter_out"],
                              inner_len=d["inner_len"] if want_inner else None, keep_failed=keep,
                              **case.common(uniform), **lay))

    o = fp.run_whole(call, in_img, out0, want, [] if case.inplace else rs, want_inp=want_inp,
                     in_ranges=rs if case.inplace else (), arrays=arrays)
    o.check(st, want_ctr[:case.count].tolist(), want_len[:case.count].tolist(), where=(*where, "open"))
    return o
