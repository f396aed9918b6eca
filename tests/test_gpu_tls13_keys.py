"""sg_tls13_traffic_keys_dev (sg_hkdf.hip) and the traffic-secret calls of the record
layer on the GPU, against tests/tls13_keys_ref.py and the host call.

Every table sits in a footprint.sentinel buffer with a margin in front and behind and is
compared whole afterwards, so a byte written outside the selected rows fails as a wrong
byte inside them does: the 4 bytes behind a 12-byte IV row (the next row's first word),
the margin behind the last row, a table the call was not given, and the secrets of a
call without UPDATE.  All comparisons are byte equality."""
from __future__ import annotations

import io

import numpy as np
import pytest

import footprint as fp
import tls13_keys_ref as R
import tls13_ref as T
from gpu_support import dev_u8, dev_u32, dev_u64, filled, host_bytes, host_np

pytestmark = pytest.mark.gpu

M = fp.MARGIN
MAX_ROWS = 257
SECRETS = R.secrets(MAX_ROWS)  # row 0 all zero, row 1 all ff, every other row's first byte has its high bit set
GENERATIONS = 3
_gen = {0: SECRETS}


def gen(g: int) -> list:
    """The secrets after g KeyUpdate steps (the reference's, computed once)."""
    if g not in _gen:
        _gen[g] = [R.next_secret(s) for s in gen(g - 1)]
    return _gen[g]


_kv: dict = {}


def key_iv(g: int, row: int):
    if (g, row) not in _kv:
        _kv[g, row] = R.traffic_keys(gen(g)[row])
    return _kv[g, row]


def table_size(rows: int, width: int) -> int:
    return M + fp.round_up(rows * width, 16) + M


class Tables:
    """The three tables of `rows` rows on the device, each inside a sentinel buffer."""

    SALTS = {"secrets": 0x21, "keys": 0x42, "ivs": 0x63}
    WIDTH = {"secrets": 32, "keys": 32, "ivs": 12}

    def __init__(self, rows: int, secrets):
        self.rows = rows
        self.start = {n: fp.sentinel(table_size(rows, w), self.SALTS[n]) for n, w in self.WIDTH.items()}
        self.start["secrets"] = self.image("secrets", dict(enumerate(secrets)))  # over the bare sentinel
        self.dev = {n: dev_u8(a) for n, a in self.start.items()}

    def image(self, name: str, rows: dict) -> np.ndarray:
        """The table's start image with the given rows laid over it."""
        w = self.WIDTH[name]
        buf = self.start[name].copy()
        for r, b in rows.items():
            assert len(b) == w and 0 <= r < self.rows
            buf[M + r * w:M + (r + 1) * w] = np.frombuffer(b, dtype=np.uint8)
        return buf

    def t(self, name: str):
        """The table itself: the rows between the device buffer's margins."""
        return self.dev[name][M:M + self.rows * self.WIDTH[name]]

    def call(self, *, keys=True, ivs=True, index=None, update=False, stream=None):
        from suruga_amd import keysched as K

        K.tls13_traffic_keys_dev(self.t("secrets"), self.t("keys") if keys else None, self.t("ivs") if ivs else None,
                                 index=None if index is None else dev_u32(index), update=update, stream=stream)

    def check(self, where, **want):
        """Every buffer, whole: want[name] = {row: bytes} over the start image (absent: untouched)."""
        import torch

        torch.cuda.synchronize()
        for name in self.WIDTH:
            w = self.WIDTH[name]
            rs = [(M + r * w, M + (r + 1) * w) for r in range(self.rows)]
            d = fp.first_diff(host_np(self.dev[name]), self.image(name, want.get(name, {})), rs)
            assert d is None, (*where, name, d)


def expected(rows, g: int, keys: bool, ivs: bool, update: bool) -> dict:
    """What a call on secrets of generation g leaves in the selected rows."""
    g2 = g + 1 if update else g
    want = {}
    if update:
        want["secrets"] = {r: gen(g2)[r] for r in rows}
    if keys:
        want["keys"] = {r: key_iv(g2, r)[0] for r in rows}
    if ivs:
        want["ivs"] = {r: key_iv(g2, r)[1] for r in rows}
    return want


@pytest.mark.parametrize("rows", (1, 63, 64, 65, 257))
@pytest.mark.parametrize("update", (False, True))
@pytest.mark.parametrize("which", ("both", "keys", "ivs"))
def test_values_and_footprint(gpu, rows, update, which):
    """rows = count: one lane, a partial wave, a wave, a wave plus one, a group plus one."""
    from suruga_amd import keysched as K

    keys, ivs = which != "ivs", which != "keys"
    tb = Tables(rows, SECRETS[:rows])
    tb.call(keys=keys, ivs=ivs, update=update)
    tb.check((rows, update, which), **expected(range(rows), 0, keys, ivs, update))
    # ... and the host call says the same as the reference
    arr = np.frombuffer(b"".join(SECRETS[:rows]), dtype=np.uint8).reshape(rows, 32)
    got = K.tls13_traffic_keys(arr, update=update, threads=3)
    g = 1 if update else 0
    assert got[0].tobytes() == b"".join(key_iv(g, r)[0] for r in range(rows))
    assert got[1].tobytes() == b"".join(key_iv(g, r)[1] for r in range(rows))
    if update:
        assert got[2].tobytes() == b"".join(gen(1)[:rows])


def test_fewer_rows_than_the_table(gpu):
    """count < rows without an index: rows 0..count-1, the rest untouched."""
    import ctypes as C

    from suruga_amd import _native as N

    tb = Tables(65, SECRETS[:65])
    k = N.SgTls13Keys()
    k.count, k.rows, k.flags = 64, 65, N.SG_TLS13_KEYS_UPDATE
    k.secrets, k.keys, k.ivs = (tb.t(n).data_ptr() for n in ("secrets", "keys", "ivs"))
    k.stream = None  # the NULL stream: the call waits
    assert gpu.sg_tls13_traffic_keys_dev(C.byref(k)) == 0
    tb.check(("count 64 of 65",), **expected(range(64), 0, True, True, True))


INDEX = [15, 0, 7, 7, 16, 0xFFFFFFFF, 3]


@pytest.mark.parametrize("update", (False, True))
def test_index_list(gpu, update):
    """16 rows; the named rows are derived, 16 and 0xFFFFFFFF are skipped, every other row of
    every table keeps its sentinel.  Under UPDATE without the duplicate, whose generation the
    interface leaves open."""
    index = [r for i, r in enumerate(INDEX) if not (update and i == 3)]
    assert (len(index), index.count(7)) == ((6, 1) if update else (7, 2))
    named = sorted({r for r in index if r < 16})
    assert named == [0, 3, 7, 15]
    tb = Tables(16, SECRETS[:16])
    tb.call(index=index, update=update)
    tb.check(("index", update), **expected(named, 0, True, True, update))


def test_generations(gpu):
    """Three UPDATE calls on the device equal three on the host; an UPDATE with neither table
    only advances the secrets."""
    from suruga_amd import keysched as K

    rows = 65
    tb = Tables(rows, SECRETS[:rows])
    host = np.frombuffer(b"".join(SECRETS[:rows]), dtype=np.uint8).reshape(rows, 32)
    for g in range(1, GENERATIONS + 1):
        tb.call(update=True)
        hk, hv, host = K.tls13_traffic_keys(host, update=True, threads=2)
        want = expected(range(rows), g - 1, True, True, True)
        tb.check(("generation", g), **want)
        assert host.tobytes() == b"".join(gen(g)[:rows])
        assert hk.tobytes() == b"".join(want["keys"][r] for r in range(rows))
        assert hv.tobytes() == b"".join(want["ivs"][r] for r in range(rows))
    tb2 = Tables(rows, SECRETS[:rows])
    tb2.call(keys=False, ivs=False, update=True)
    tb2.check(("update alone",), secrets={r: gen(1)[r] for r in range(rows)})


def test_keys_then_seal_on_one_stream(gpu):
    """A KeyUpdate of 4 connections and a TLS 1.3 seal under the new rows, enqueued back to
    back on one stream with no host wait in between: the fragments are the reference's under
    generation 1, and none of them opens under the old tables."""
    import torch

    from suruga_amd import batch as B
    from suruga_amd import keysched as K

    rows = 4
    lens = [64, 100] * 4
    kidx = [i % rows for i in range(len(lens))]
    seqs = [5 + 3 * i for i in range(len(lens))]
    contents = [np.random.default_rng([i, n]).bytes(n) for i, n in enumerate(lens)]
    in_off = np.arange(len(lens), dtype=np.uint64) * 128
    out_off = np.arange(len(lens), dtype=np.uint64) * 128
    inp = np.zeros(128 * len(lens), dtype=np.uint8)
    for o, c in zip(in_off, contents):
        inp[int(o):int(o) + len(c)] = np.frombuffer(c, dtype=np.uint8)

    tb = Tables(rows, SECRETS[2:2 + rows])  # SHAKE rows
    old_keys, old_ivs = K.tls13_traffic_keys(np.frombuffer(b"".join(SECRETS[2:2 + rows]), dtype=np.uint8).reshape(rows, 32))
    common = dict(count=len(lens), key_index=dev_u32(kidx), seq=dev_u64(seqs), content_type=23)
    d_in, d_out = dev_u8(inp), filled(128 * len(lens), 0xEE)
    seal_args = dict(common, lens=dev_u32(lens), max_len=max(lens), in_off=dev_u64(in_off), out_off=dev_u64(out_off))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # the uploads are done; from here on nothing waits until both calls are enqueued
    tb.call(update=True, stream=stream)
    B.seal_tls13(B.Batch(keys=tb.t("keys").view(rows, 32), ivs=tb.t("ivs"), inp=d_in, out=d_out, stream=stream,
                         **seal_args))
    stream.synchronize()
    out_h = host_bytes(d_out)
    frags = []
    for i, (c, k, q) in enumerate(zip(contents, kidx, seqs)):
        key, iv = R.traffic_keys(R.next_secret(SECRETS[2 + k]))
        want = T.seal(key, iv, q, c, 23)
        o = int(out_off[i])
        assert out_h[o:o + len(want)] == want, ("record", i)
        frags.append(want)
    tb.check(("stream",), secrets={r: R.next_secret(SECRETS[2 + r]) for r in range(rows)},
             keys={r: R.traffic_keys(R.next_secret(SECRETS[2 + r]))[0] for r in range(rows)},
             ivs={r: R.traffic_keys(R.next_secret(SECRETS[2 + r]))[1] for r in range(rows)})

    def open_under(keys_t, ivs_t):
        st, ty, cl = filled(len(lens), 0xFF), filled(len(lens), 0xFF), dev_u32([0xFFFFFFFF] * len(lens))
        flens = [len(f) for f in frags]
        B.open_tls13(B.Batch(keys=keys_t, ivs=ivs_t, inp=d_out, out=filled(128 * len(lens), 0xDD), status=st, inner_type=ty,
                             content_len=cl, lens=dev_u32(flens), max_len=max(flens), in_off=dev_u64(out_off),
                             out_off=dev_u64(in_off), **common))
        torch.cuda.synchronize()
        return list(host_bytes(st)), host_np(cl).view(np.uint32).tolist()

    assert open_under(dev_u8(old_keys.reshape(-1)).view(rows, 32), dev_u8(old_ivs.reshape(-1))) == (
        [T.BAD_MAC] * len(lens), [0] * len(lens))
    assert open_under(tb.t("keys").view(rows, 32), tb.t("ivs")) == ([T.OK] * len(lens), lens)


# ---------------------------------------------------------------------------
# the record layer: a context made from a secret, and the stream classes
# ---------------------------------------------------------------------------
SECRET = SECRETS[5]
MESSAGES = [(23, b"first write of generation 0"), (23, bytes(range(200))), None,
            (23, b"after the update"), (21, b"\x01\x00")]


def reference_wire(request_update: bool = True):
    """The five records: sequence 0, 1, 2 under generation 0 (the third is the KeyUpdate),
    then 0, 1 under generation 1."""
    from suruga_amd.tls13 import key_update_message

    records, g, seq = [], 0, 0
    for m in MESSAGES:
        ctype, content = m if m is not None else (22, key_update_message(request_update))
        key, iv = R.traffic_keys(R.generation(SECRET, g))
        frag = T.seal(key, iv, seq, content, ctype)
        records.append(T.header(len(frag)) + frag)
        seq += 1
        if m is None:
            g, seq = g + 1, 0
    return records


def write_all(wr):
    for m in MESSAGES:
        if m is None:
            wr.send_key_update(True)
        else:
            wr.write_data(*m)


def test_writer_follows_a_key_update(gpu):
    from suruga_amd.tls13 import Tls13Writer, key_update_message

    sink = io.BytesIO()
    wr = Tls13Writer.from_secret(sink, SECRET)
    try:
        write_all(wr)
        assert wr.write_count == 2
    finally:
        wr.close()
    want = reference_wire()
    wire, pos = sink.getvalue(), 0
    for i, rec in enumerate(want):
        assert wire[pos:pos + len(rec)] == rec, ("record", i)
        pos += len(rec)
    assert pos == len(wire)
    assert key_update_message(True) == bytes.fromhex("1800000101") and key_update_message(False) == bytes.fromhex("1800000100")


def delivered():
    from suruga_amd.tls13 import key_update_message

    return [m if m is not None else (22, key_update_message(True)) for m in MESSAGES]


def test_reader_follows_a_key_update_inside_one_buffer(gpu):
    from suruga_amd.tls13 import Tls13StreamReader

    rd = Tls13StreamReader.from_secret(SECRET)
    try:
        assert rd.key_update_requested is False
        rd.feed(b"".join(reference_wire()))
        assert rd.drain() == delivered()
        assert rd.key_update_requested is True and rd.read_count == 2 and not rd.buf
        assert rd.drain() == []
    finally:
        rd.close()


def test_reader_follows_a_key_update_across_buffers(gpu):
    """The KeyUpdate is the last record of one buffer, the next generation's records come
    later; and an update that asks for none in return leaves key_update_requested alone."""
    from suruga_amd.tls13 import Tls13StreamReader

    recs = reference_wire(request_update=False)
    rd = Tls13StreamReader.from_secret(SECRET)
    try:
        rd.feed(b"".join(recs[:3]) + recs[3][:7])
        assert [t for t, _ in rd.drain()] == [23, 23, 22] and rd.read_count == 0 and len(rd.buf) == 7
        rd.feed(recs[3][7:] + recs[4])
        assert rd.drain() == delivered()[3:] and rd.read_count == 2
        assert rd.key_update_requested is False
    finally:
        rd.close()


def test_reader_from_a_secret_still_raises_on_a_bad_record(gpu):
    """An error whose preceding record is not a KeyUpdate raises as before."""
    from suruga_amd.cipher import TlsError, TlsErrorKind
    from suruga_amd.tls13 import Tls13StreamReader

    recs = reference_wire()
    bad = bytearray(recs[1])
    bad[-1] ^= 1
    rd = Tls13StreamReader.from_secret(SECRET)
    try:
        rd.feed(recs[0] + bytes(bad) + recs[2])
        with pytest.raises(TlsError) as e:
            rd.drain()
        assert e.value.kind == TlsErrorKind.BadRecordMac and rd.read_count == 1
    finally:
        rd.close()


def test_plain_reader_stops_at_the_key_change(gpu):
    """A reader made from key and IV delivers the three records of generation 0 and raises
    BadRecordMac at the fourth, as it always did."""
    from suruga_amd import _native as N
    from suruga_amd.cipher import TlsError, TlsErrorKind
    from suruga_amd.tls13 import Tls13StreamReader, Tls13Writer

    key, iv = R.traffic_keys(SECRET)
    rd = Tls13StreamReader(key, iv)
    try:
        rd.feed(b"".join(reference_wire()))
        with pytest.raises(TlsError) as e:
            rd.drain()
        assert e.value.kind == TlsErrorKind.BadRecordMac and rd.read_count == 3
        with pytest.raises(N.NativeError) as ne:
            rd.key_update()  # no secret to ratchet
        assert ne.value.code == N.SG_E_ARG and rd.read_count == 3
    finally:
        rd.close()
    # a writer from key and IV writes generation 0's bytes, and cannot update either
    sink = io.BytesIO()
    wr = Tls13Writer(sink, key, iv)
    try:
        wr.write_data(*MESSAGES[0])
        assert sink.getvalue() == reference_wire()[0]
        with pytest.raises(N.NativeError):
            wr.send_key_update()
    finally:
        wr.close()


def test_context_calls(gpu):
    """sg_ctx_key_update needs a secret; sg_ctx_set_traffic_secret on an existing context
    replaces its key and IV, and sg_ctx_set_iv keeps working beside it."""
    import ctypes as C

    from suruga_amd import _native as N

    ctx = gpu.sg_ctx_new(bytes(32), 0)
    assert ctx
    try:
        assert gpu.sg_ctx_key_update(ctx) == N.SG_E_ARG and b"secret" in gpu.sg_last_error()
        assert gpu.sg_ctx_set_traffic_secret(ctx, SECRET) == 0
        assert gpu.sg_ctx_key_update(ctx) == 0

        def write(seq, content):
            wire = (C.c_uint8 * gpu.sg_wire_bound_tls13(len(content)))()
            wl = C.c_size_t(0)
            src = (C.c_uint8 * len(content)).from_buffer_copy(content)
            assert gpu.sg_write_records_tls13(ctx, seq, 23, src, len(content), wire, len(wire), C.byref(wl)) == 1
            return bytes(wire)[:wl.value]

        key, iv = R.traffic_keys(R.generation(SECRET, 1))
        frag = T.seal(key, iv, 9, b"generation one", 23)
        assert write(9, b"generation one") == T.header(len(frag)) + frag
        other = bytes(range(100, 112))
        assert gpu.sg_ctx_set_iv(ctx, other) == 0  # the key stays, the IV is the caller's
        frag = T.seal(key, other, 0, b"own iv", 23)
        assert write(0, b"own iv") == T.header(len(frag)) + frag
    finally:
        gpu.sg_ctx_free(ctx)
