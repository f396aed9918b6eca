"""What the IPsec ESP tests share -- TEST INFRASTRUCTURE ONLY.

* ``Pkt`` / ``EspCase``: a batch on the host -- every payload, its sequence number, IV, next
  header and SA, and where it lies -- with the reference's (tests/esp_ref.py) packets,
  computed once.  A ``Pkt`` with ``plain`` set is a packet with that AEAD plaintext, trailer
  and all, for the trailers no seal writes; such a case is only opened.
* whole-buffer runs: every device buffer starts as footprint.sentinel with a margin in
  front and behind and the *whole* buffer, the status bytes, seq_out, payload_len and
  next_header_out are compared afterwards, so a stray write, an unwritten padding byte or a
  seq_out that a seal touched fails as a wrong byte does.  A payload's slot holds its
  padded length, so the input of a seal has sentinel bytes directly behind len_i: an output
  that depended on them would differ from the reference's.  In place (``inplace=True``)
  there is one buffer: packet i at its offset, its payload 16 bytes behind that.

Imports without torch and without a GPU."""
from __future__ import annotations

import hashlib
from dataclasses import dataclass

import numpy as np

import esp_ref as E
import footprint as fp
import rfc8439_ref as R
from quic_support import offsets
from wg_support import SPARE, layout_args

M = fp.MARGIN
# four SAs; row r sits at SEQ_EDGES[r], the top of its window, so every edge is inferred under ESN
KEYS4 = R.KEYS + hashlib.sha256(b"esp key 3").digest()
SALTS4 = b"".join(hashlib.sha256(b"esp salt %d" % i).digest()[:4] for i in range(4))
SPIS4 = (0x01020304, 0xFFFFFFFF, 0x80000001, 0x00000100)
SEQ_EDGES = (0, 2**32 - 1, 2**32, 2**64 - 1)
WINDOW = 64
NEXT_HEADERS = (4, 41, 59, 255, 0, 6)


def rnd(n: int, what: str) -> bytes:
    return R.data(n, what.encode())


@dataclass
class Pkt:
    payload: bytes
    seq: int
    kidx: int = 0
    nh: int = 4
    iv: object = None     # None: the sequence number
    plain: object = None  # the whole AEAD plaintext instead of payload, padding and trailer


class EspCase:
    """Payloads with a table of SAs.  A payload's slot holds its padded length, a packet's
    slot 32 bytes more."""

    def __init__(self, pkts, keys=KEYS4, salts=SALTS4, spis=SPIS4, align=4, esn=False, tops=SEQ_EDGES, window=WINDOW,
                 in_skew=lambda i: i % 16, out_skew=lambda i: (i // 16 + 5 * i) % 16, strides=None, inplace=False):
        """The packets lie one behind the other at a multiple of 16 plus the skews -- every pair
        of skews within 256 packets -- or, with strides = (payload stride, payload base, packet
        stride, packet base), at equal distances, as the uniform fields need them."""
        self.pkts, self.keys, self.salts, self.spis = list(pkts), keys, salts, tuple(spis)
        self.align, self.esn, self.tops, self.window, self.inplace = align, esn, tuple(tops), window, inplace
        self.count = len(self.pkts)
        self.num_sas = len(keys) // 32
        assert len(self.spis) == self.num_sas == len(salts) // 4 == len(self.tops)
        self.lens = np.array([len(p.payload) for p in self.pkts], dtype=np.uint32)
        self.padded = np.array([len(p.plain) if p.plain is not None else E.padded_len(len(p.payload), align)
                                for p in self.pkts], dtype=np.uint32)
        self.pkt_lens = self.padded + np.uint32(32)
        if strides is None:
            self.msg_off, self.msg_size = offsets(self.pkt_lens, out_skew)
            self.raw_off, self.raw_size = offsets(self.padded, in_skew)
        else:
            si, bi, so, bo = strides
            assert si >= int(self.padded.max()) and so >= int(self.pkt_lens.max())
            self.raw_off = np.arange(self.count, dtype=np.uint64) * np.uint64(si) + np.uint64(bi)
            self.msg_off = np.arange(self.count, dtype=np.uint64) * np.uint64(so) + np.uint64(bo)
            self.raw_size, self.msg_size = fp.round_up(bi + si * self.count, 16), fp.round_up(bo + so * self.count, 16)
        if inplace:
            self.raw_off, self.raw_size = self.msg_off + np.uint64(16), self.msg_size
        self._protected = {}

    def row(self, i) -> int:
        return min(self.pkts[i].kidx, self.num_sas - 1)

    def sa(self, i):
        """(key, salt, spi) of packet i."""
        r = self.row(i)
        return self.keys[32 * r:32 * r + 32], self.salts[4 * r:4 * r + 4], self.spis[r]

    def seq(self, i) -> int:
        """The sequence number as the packet carries it."""
        return self.pkts[i].seq if self.esn else self.pkts[i].seq & E.M32

    def protected(self, i) -> bytes:
        """The reference's packet i, computed once."""
        if i not in self._protected:
            p = self.pkts[i]
            if p.plain is not None:
                self._protected[i] = E.protect_plain(*self.sa(i), p.seq, p.plain, esn=self.esn, iv=p.iv)
            else:
                self._protected[i] = E.protect(*self.sa(i), p.seq, p.payload, p.nh, align=self.align, esn=self.esn, iv=p.iv)
        return self._protected[i]

    def opened(self, i, pkt: bytes, want_trailer=True, bound=E.MAX_PACKET_LEN, tops=None):
        return E.unprotect(*self.sa(i), pkt, esn=self.esn, top=(tops or self.tops)[self.row(i)], window=self.window,
                           want_trailer=want_trailer, max_len=bound)

    # ---- device arguments
    def common(self, uniform=False) -> dict:
        from gpu_support import dev_bytes, dev_u32

        c = dict(count=self.count, keys=dev_bytes(self.keys), salts=dev_bytes(self.salts), spi=dev_u32(self.spis),
                 esn=self.esn)
        if uniform:
            assert all(p.kidx == 0 for p in self.pkts)
        else:
            c["sa_index"] = dev_u32([p.kidx for p in self.pkts])
        return c


def _arrays(count):
    return {"status": fp.array_start(count, 0x51), "seq_out": fp.array_start(count, 0x52, np.uint64),
            "payload_len": fp.array_start(count, 0x53, np.uint32), "next_header_out": fp.array_start(count, 0x54)}


def seal_whole(case: EspCase, *, uniform=False, max_len=None, exp_st=None, where=(), stream=None):
    """Seal into a sentinel buffer with margins: the whole output is the sentinel with every
    packet of the reference laid over it (nothing for a status 3), the input is unchanged --
    in place: the one buffer is that image -- the statuses are exp_st (default: all 0) and
    seq_out, payload_len and next_header_out, which a seal does not read, are untouched.
    uniform: no per-packet array at all -- one length, one next header, the IV the sequence
    number, SA 0 -- but seq, which a seal always takes."""
    from gpu_support import dev_u8, dev_u64
    from suruga_amd import esp as ESP

    assert all(p.plain is None for p in case.pkts)
    exp_st = [0] * case.count if exp_st is None else exp_st
    payloads = [(M + int(o), p.payload) for o, p in zip(case.raw_off, case.pkts)]
    msgs = [(M + int(case.msg_off[i]), case.protected(i)) for i in range(case.count) if exp_st[i] == 0]
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.msg_off, case.pkt_lens)]
    lay, bi, bo = layout_args(case.lens, case.raw_off, case.msg_off, uniform, max_len)
    per = dict(seq=dev_u64([p.seq for p in case.pkts]))
    if uniform:
        assert all(p.iv is None and p.nh == case.pkts[0].nh for p in case.pkts)
        per["uniform_next_header"] = case.pkts[0].nh
    else:
        per["next_header"] = dev_u8(np.array([p.nh for p in case.pkts], dtype=np.uint8))
        if any(p.iv is not None for p in case.pkts):
            per["iv"] = dev_u64([case.seq(i) if p.iv is None else p.iv for i, p in enumerate(case.pkts)])
    size = M + case.msg_size + M
    if case.inplace:
        in_img, out0, want = fp.image(size, 0x5A, payloads), fp.sentinel(SPARE, 0x77), fp.sentinel(SPARE, 0x77)
        # a skipped packet keeps its payload; every other slot becomes its packet
        want_inp = fp.image(size, 0x5A, [x for i, x in enumerate(payloads) if exp_st[i] != 0] + msgs)
        pick = lambda d: (d["inp"][M + bi:], d["inp"][M + bo:])  # noqa: E731
    else:
        in_img, out0 = fp.image(M + case.raw_size + M, 0x31, payloads), fp.sentinel(size, 0x5A)
        want, want_inp = fp.image(size, 0x5A, msgs), None
        pick = lambda d: (d["inp"][M + bi:], d["out"][M + bo:])  # noqa: E731

    def call(d):
        inp, out = pick(d)
        ESP.seal_esp(ESP.EspBatch(inp=inp, out=out, status=d["status"], align=case.align, seq_out=d["seq_out"],
                                  payload_len=d["payload_len"], next_header_out=d["next_header_out"], stream=stream,
                                  **per, **case.common(uniform), **lay))

    o = fp.run_whole(call, in_img, out0, want, [] if case.inplace else rs, want_inp=want_inp,
                     in_ranges=rs if case.inplace else (), arrays=_arrays(case.count))
    o.check(exp_st, None, None, None, where=(*where, "seal"))
    return o


def open_whole(case: EspCase, msgs=None, *, lens=None, keep=False, uniform=False, max_len=None, want_trailer=True,
               tops=None, where=()):
    """Open msgs (default: the reference's packets), laid out like the seal's output, into a
    sentinel buffer -- in place: where they lie, 16 bytes on.  Per packet, as the reference
    (esp_ref.unprotect) says: the whole output is the decryption with its trailer (status 0 and
    7), zeros and seq_out 0 (status 1), the decryption and the inferred sequence number (status
    1 with keep), or nothing, the arrays included (status 2, 3, 6).  want_trailer=False:
    payload_len and next_header_out are NULL and their arrays stay as they were.  tops: the
    replay_top table of this call, where it is not the case's."""
    from gpu_support import dev_u64
    from suruga_amd import esp as ESP

    tops = tuple(case.tops if tops is None else tops)
    msgs = [case.protected(i) for i in range(case.count)] if msgs is None else msgs
    lens = np.array([len(m) for m in msgs], dtype=np.uint32) if lens is None else np.asarray(lens, dtype=np.uint32)
    bound = int(lens.max()) if max_len is None else max_len
    placed = [(M + int(o), m) for o, m in zip(case.msg_off, msgs)]
    arrays = _arrays(case.count)
    st, parts = [], []
    want_seq, want_len, want_nh = arrays["seq_out"].copy(), arrays["payload_len"].copy(), arrays["next_header_out"].copy()
    for i in range(case.count):
        rc, pt, seq, n, nh = case.opened(i, msgs[i][:int(lens[i])], want_trailer, bound, tops)
        st.append(rc)
        if pt is None:
            continue
        scrub = rc == 1 and not keep
        parts.append((M + int(case.raw_off[i]), bytes(len(pt)) if scrub else pt))
        want_seq[i] = 0 if scrub else seq
        if want_trailer:
            want_len[i], want_nh[i] = n, nh
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
    esn_args = dict(replay_top=dev_u64(tops), window=case.window) if case.esn else {}

    def call(d):
        inp, out = pick(d)
        ESP.open_esp(ESP.EspBatch(inp=inp, out=out, status=d["status"], seq_out=d["seq_out"],
                                  payload_len=d["payload_len"] if want_trailer else None,
                                  next_header_out=d["next_header_out"] if want_trailer else None, keep_failed=keep,
                                  **esn_args, **case.common(uniform), **lay))

    o = fp.run_whole(call, in_img, out0, want, [] if case.inplace else rs, want_inp=want_inp,
                     in_ranges=rs if case.inplace else (), arrays=arrays)
    o.check(st, want_seq[:case.count].tolist(), want_len[:case.count].tolist(), want_nh[:case.count].tolist(),
            where=(*where, "open"))
    return o
