"""What the DTLS 1.3 tests share -- TEST INFRASTRUCTURE ONLY.

* ``Rec`` / ``DtlsCase``: a batch on the host -- every content, its sequence number, type,
  epoch and connection, the header's form and where everything lies -- with the reference's
  (tests/dtls13_ref.py) records, computed once.  A ``Rec`` with ``inner`` set is a record with
  that inner plaintext, for the inner plaintexts no seal writes; such a case is only opened.
* whole-buffer runs: every device buffer starts as footprint.sentinel with a margin in
  front and behind and the *whole* buffer, the status bytes, seq_out, epoch_out, content_len
  and type_out are compared afterwards, so a stray write, an unwritten padding byte or a
  seq_out that a seal touched fails as a wrong byte does.  A content's slot holds its inner
  plaintext's length, so the input of a seal has sentinel bytes directly behind len_i: an
  output that depended on them would differ from the reference's.

Imports without torch and without a GPU."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import dtls13_ref as D
import footprint as fp
import rfc8439_ref as R
from quic_support import offsets
from wg_support import layout_args

M = fp.MARGIN
ROWS = 8  # three connections, or two connections of four epochs each
KEYS = R.data(32 * ROWS, b"dtls13 test keys")
IVS = R.data(12 * ROWS, b"dtls13 test ivs")
SNS = R.data(32 * ROWS, b"dtls13 test sn keys")
TYPES = (23, 22, 21, 26, 1, 255)


def rnd(n: int, what: str) -> bytes:
    return R.data(n, what.encode())


@dataclass
class Rec:
    content: bytes
    seq: int
    kidx: int = 0
    ctype: int = 23
    epoch: int = 0
    inner: object = None  # the whole inner plaintext instead of content, type and padding


class DtlsCase:
    """Contents with tables of connections.  A content's slot holds its inner plaintext's
    length, a record's slot header and tag more."""

    def __init__(self, recs, *, cid_len=0, seq16=False, length=False, pad_to=0, epoch_rows=False, expected=0, tables=None,
                 in_skew=lambda i: i % 16, out_skew=lambda i: (i // 16 + 5 * i) % 16, strides=None):
        """expected: one number for every row, or one per row.  tables: (keys, ivs, sn_keys, cids)
        of three connections in place of the module's.  The records lie one behind the
        other at a multiple of 16 plus the skews, or, with strides = (content stride, content
        base, record stride, record base), at equal distances, as the uniform fields need them."""
        self.recs = list(recs)
        self.cid_len, self.seq16, self.length, self.pad_to, self.epoch_rows = cid_len, seq16, length, pad_to, epoch_rows
        self.num_conns = 2 if epoch_rows else 3
        self.rows = 4 * self.num_conns if epoch_rows else self.num_conns
        self.keys, self.ivs, self.sns = KEYS[:32 * self.rows], IVS[:12 * self.rows], SNS[:32 * self.rows]
        self.cids = rnd(cid_len * self.num_conns, f"dtls13 test cids {cid_len}")
        if tables is not None:
            assert not epoch_rows
            self.keys, self.ivs, self.sns, self.cids = tables
            assert len(self.keys) == 32 * self.rows and len(self.cids) == cid_len * self.num_conns
        self.expected = [expected] * self.rows if isinstance(expected, int) else list(expected)
        assert len(self.expected) == self.rows
        self.count = len(self.recs)
        self.hdr_len = D.header_len(seq16, length, cid_len)
        self.lens = np.array([len(r.content) for r in self.recs], dtype=np.uint32)
        self.inner = np.array([len(r.inner) if r.inner is not None else D.inner_len(len(r.content), pad_to)
                               for r in self.recs], dtype=np.uint32)
        self.rec_lens = self.inner + np.uint32(self.hdr_len + 16)
        if strides is None:
            self.rec_off, self.rec_size = offsets(self.rec_lens, out_skew)
            self.raw_off, self.raw_size = offsets(self.inner, in_skew)
        else:
            si, bi, so, bo = strides
            assert si >= int(self.inner.max()) and so >= int(self.rec_lens.max())
            self.raw_off = np.arange(self.count, dtype=np.uint64) * np.uint64(si) + np.uint64(bi)
            self.rec_off = np.arange(self.count, dtype=np.uint64) * np.uint64(so) + np.uint64(bo)
            self.raw_size, self.rec_size = fp.round_up(bi + si * self.count, 16), fp.round_up(bo + so * self.count, 16)
        self._protected = {}

    def conn(self, i) -> int:
        return min(self.recs[i].kidx, self.num_conns - 1)

    def row_of(self, conn: int, ee: int) -> int:
        return 4 * conn + ee if self.epoch_rows else conn

    def table_row(self, row: int, expected=None):
        """(key, iv, sn_key, expected) of a row."""
        e = self.expected if expected is None else expected
        return self.keys[32 * row:32 * row + 32], self.ivs[12 * row:12 * row + 12], self.sns[32 * row:32 * row + 32], e[row]

    def cid(self, i) -> bytes:
        c = self.conn(i)
        return self.cids[self.cid_len * c:self.cid_len * (c + 1)]

    def protected(self, i) -> bytes:
        """The reference's record i, computed once."""
        if i not in self._protected:
            r = self.recs[i]
            key, iv, sn, _ = self.table_row(self.row_of(self.conn(i), r.epoch & 3))
            form = dict(epoch=r.epoch, cid=self.cid(i), seq16=self.seq16, length=self.length)
            if r.inner is not None:
                self._protected[i] = D.protect_inner(key, iv, sn, r.seq, r.inner, **form)
            else:
                self._protected[i] = D.protect(key, iv, sn, r.seq, r.content, r.ctype, pad_to=self.pad_to, **form)
        return self._protected[i]

    def opened(self, i, rec: bytes, bound=D.MAX_RECORD_LEN, expected=None):
        c = self.conn(i)
        return D.unprotect(lambda ee: self.table_row(self.row_of(c, ee), expected), rec, self.cid_len, max_len=bound)

    # ---- device arguments
    def common(self, uniform=False) -> dict:
        from gpu_support import dev_bytes, dev_u32

        c = dict(count=self.count, keys=dev_bytes(self.keys), ivs=dev_bytes(self.ivs), sn_keys=dev_bytes(self.sns),
                 cid_len=self.cid_len, epoch_rows=self.epoch_rows)
        if uniform:
            assert all(r.kidx == 0 for r in self.recs)
        else:
            c["key_index"] = dev_u32([r.kidx for r in self.recs])
        return c


def _arrays(count):
    return {"status": fp.array_start(count, 0x51), "seq_out": fp.array_start(count, 0x52, np.uint64),
            "epoch_out": fp.array_start(count, 0x53), "content_len": fp.array_start(count, 0x54, np.uint32),
            "type_out": fp.array_start(count, 0x55)}


def seal_whole(case: DtlsCase, *, uniform=False, max_len=None, exp_st=None, where=(), stream=None):
    """Seal into a sentinel buffer with margins: the whole output is the sentinel with every
    record of the reference laid over it (nothing for a status 3), the input is unchanged, the
    statuses are exp_st (default: all 0) and the arrays an open writes, which a seal does not
    read, are untouched.  uniform: no per-record array at all -- one length, one type, one
    epoch, connection 0 -- but seq, which a seal always takes."""
    from gpu_support import dev_bytes, dev_u8, dev_u64
    from suruga_amd import dtls13 as DT

    assert all(r.inner is None for r in case.recs)
    exp_st = [0] * case.count if exp_st is None else exp_st
    contents = [(M + int(o), r.content) for o, r in zip(case.raw_off, case.recs)]
    recs = [(M + int(case.rec_off[i]), case.protected(i)) for i in range(case.count) if exp_st[i] == 0]
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.rec_off, case.rec_lens)]
    lay, bi, bo = layout_args(case.lens, case.raw_off, case.rec_off, uniform, max_len)
    per = dict(seq=dev_u64([r.seq for r in case.recs]), pad_to=case.pad_to, seq16=case.seq16, length=case.length)
    if case.cid_len:
        per["cids"] = dev_bytes(case.cids)
    if uniform:
        assert all(r.ctype == case.recs[0].ctype and r.epoch == case.recs[0].epoch for r in case.recs)
        per["uniform_type"], per["uniform_epoch"] = case.recs[0].ctype, case.recs[0].epoch
    else:
        per["type"] = dev_u8(np.array([r.ctype for r in case.recs], dtype=np.uint8))
        per["epoch"] = dev_u8(np.array([r.epoch & 0xFF for r in case.recs], dtype=np.uint8))
    size = M + case.rec_size + M
    in_img, out0 = fp.image(M + case.raw_size + M, 0x31, contents), fp.sentinel(size, 0x5A)
    want = fp.image(size, 0x5A, recs)

    def call(d):
        DT.seal_dtls13(DT.Dtls13Batch(inp=d["inp"][M + bi:], out=d["out"][M + bo:], status=d["status"], seq_out=d["seq_out"],
                                      epoch_out=d["epoch_out"], content_len=d["content_len"], type_out=d["type_out"],
                                      stream=stream, **per, **case.common(uniform), **lay))

    o = fp.run_whole(call, in_img, out0, want, rs, arrays=_arrays(case.count))
    o.check(exp_st, None, None, None, None, where=(*where, "seal"))
    return o


def open_whole(case: DtlsCase, msgs=None, *, lens=None, keep=False, uniform=False, max_len=None, expected=None, where=()):
    """Open msgs (default: the reference's records), laid out like the seal's output, into a
    sentinel buffer.  Per record, as the reference (dtls13_ref.unprotect) says: the whole
    output is the inner plaintext (status 0 and 5), zeros with seq_out, content_len and
    type_out 0 (status 1), the decryption and the decoded sequence number (status 1 with
    keep), or nothing, the arrays included (status 2, 3, 6).  expected: the table of this
    call, where it is not the case's."""
    from gpu_support import dev_u64
    from suruga_amd import dtls13 as DT

    expected = list(case.expected if expected is None else expected)
    msgs = [case.protected(i) for i in range(case.count)] if msgs is None else msgs
    lens = np.array([len(m) for m in msgs], dtype=np.uint32) if lens is None else np.asarray(lens, dtype=np.uint32)
    bound = int(lens.max()) if max_len is None else max_len
    placed = [(M + int(o), m) for o, m in zip(case.rec_off, msgs)]
    arrays = _arrays(case.count)
    want = {k: v.copy() for k, v in arrays.items() if k != "status"}
    st, parts = [], []
    for i in range(case.count):
        rc, inner, seq, ee, clen, ctype = case.opened(i, msgs[i][:int(lens[i])], bound, expected)
        st.append(rc)
        if inner is None:
            continue
        scrub = rc == 1 and not keep
        parts.append((M + int(case.raw_off[i]), bytes(len(inner)) if scrub else inner))
        want["seq_out"][i], want["epoch_out"][i] = 0 if scrub else seq, ee
        want["content_len"][i], want["type_out"][i] = clen, ctype
    rs = [(M + int(o), M + int(o) + int(n)) for o, n in zip(case.raw_off, case.inner)]
    lay, bi, bo = layout_args(lens, case.rec_off, case.raw_off, uniform, max_len)
    in_img, out_size = fp.image(M + case.rec_size + M, 0x33, placed), M + case.raw_size + M
    out0, want_out = fp.sentinel(out_size, 0xA5), fp.image(out_size, 0xA5, parts)

    def call(d):
        DT.open_dtls13(DT.Dtls13Batch(inp=d["inp"][M + bi:], out=d["out"][M + bo:], status=d["status"], seq_out=d["seq_out"],
                                      epoch_out=d["epoch_out"], content_len=d["content_len"], type_out=d["type_out"],
                                      expected=dev_u64(expected), keep_failed=keep, **case.common(uniform), **lay))

    o = fp.run_whole(call, in_img, out0, want_out, rs, arrays=arrays)
    o.check(st, *(want[k][:case.count].tolist() for k in ("seq_out", "epoch_out", "content_len", "type_out")),
            where=(*where, "open"))
    return o
