"""sg_seal_batch_dtls13 / sg_open_batch_dtls13 on the GPU against tests/dtls13_ref.py.

Every case is a batch of a few dozen records at most on sentinel buffers
(dtls13_support.seal_whole / open_whole): the whole output buffer, the input and every
per-record array are compared, so a byte written outside a record, an input byte read
beyond len_i that changed the output, or an array a call should not touch fails like a
wrong byte.  Records lie back to back at every pair of address skews mod 16."""
from __future__ import annotations

import hashlib

import numpy as np
import pytest

import dtls13_ref as D
import mac_forge as mf
import quic_model as QM
import quic_support as QS
import rfc8439_ref as R
import rfc_batch_support as RB
from dtls13_support import IVS, KEYS, TYPES, DtlsCase, Rec, open_whole, rnd, seal_whole
from gpu_support import dev_bytes, dev_u8, dev_u32, dev_u64, filled, host_bytes, host_np

pytestmark = pytest.mark.gpu

BASE = 2**40 + 1000  # the expected number of every row unless a test says otherwise
FORMS = ((False, False), (False, True), (True, False), (True, True))  # (16-bit sequence number, length field)
CID_LENS = (0, 1, 11, 12, 250)  # 11 and 12: with both options the header is 16 and 17 bytes
SMALL = (0, 1, 14, 15, 16, 47, 62, 63, 64, 65, 127, 128, 8 * 64 - 1, 8 * 64, 2031)
BIG = SMALL + (2049, 16 * 64 - 1, 16 * 64, 16384)


def parity_records(lengths, what: str, near=BASE, spread=100):
    """One record per length and a second of every third, over the connections, types and epochs."""
    ls = list(lengths) + list(lengths)[::3]
    return [Rec(rnd(n, f"dtls13 {what} {i}"), near - spread + (7 * i) % (2 * spread), kidx=i % 4, ctype=TYPES[i % 6], epoch=i % 5)
            for i, n in enumerate(ls)]


@pytest.mark.parametrize("form", FORMS)
def test_fixture_parity(gpu, form):
    """The fixture's records (OpenSSL's) of one header form, byte for byte, seal and open.  The
    reference is held against the stored header, tag and ciphertext hash here as well."""
    g = D.golden()
    key, iv, sn = (bytes.fromhex(g[k]) for k in ("key", "iv", "sn_key"))
    groups = {}
    for c in g["cases"]:
        groups.setdefault((c["seq16"], c["length"], c["cid_len"], c["pad_to"]), []).append(c)
    seqs = sorted({c["seq"] for c in g["cases"]})
    assert len(seqs) == 3
    assert {k[:2] for k in groups} == set(FORMS)
    for (seq16, length, cid_len, pad_to), cs in groups.items():
        if (seq16, length) != form:
            continue
        tables = (key * 3, iv * 3, sn * 3, R.data(cid_len, b"dtls13 cid %d" % cid_len) * 3)
        recs = [Rec(R.data(c["n"], b"dtls13 content %d" % c["n"]), c["seq"], kidx=seqs.index(c["seq"]), ctype=c["type"],
                    epoch=c["epoch"]) for c in cs]
        case = DtlsCase(recs, cid_len=cid_len, seq16=seq16, length=length, pad_to=pad_to, expected=seqs, tables=tables)
        for i, c in enumerate(cs):
            rec, hl = case.protected(i), case.hdr_len
            assert (rec[:1] + rec[1 + cid_len:hl]).hex() == c["protected_header"] and rec[-16:].hex() == c["tag"]
            assert hashlib.sha256(rec[hl:-16]).hexdigest() == c["ct_sha256"] and len(rec) == hl + c["inner"] + 16
        where = ("fixture", seq16, length, cid_len, pad_to)
        seal_whole(case, max_len=16384, where=where)
        o = open_whole(case, max_len=D.MAX_RECORD_LEN, where=where)
        assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count


@pytest.mark.parametrize("cid_len", CID_LENS)
@pytest.mark.parametrize("seq16,length", FORMS)
@pytest.mark.parametrize("which", ("small", "big"))
def test_parity_per_record_arrays(gpu, which, seq16, length, cid_len):
    """Whole-buffer parity with per-record arrays, 8 lanes (max_len at most 2 KiB) and 16.
    Open's bound is on the record: under 2,048 the records of 2,031 content bytes, and with
    the longest header a few more, are skipped and left untouched; the big set opens them."""
    case = DtlsCase(parity_records(SMALL if which == "small" else BIG, f"parity {which}"), cid_len=cid_len, seq16=seq16,
                    length=length, expected=BASE)
    where = (which, seq16, length, cid_len)
    seal_whole(case, max_len=2031 if which == "small" else 16384, where=where)
    bound = 2048 if which == "small" else D.MAX_RECORD_LEN
    o = open_whole(case, max_len=bound, where=where)
    assert o.arrays["status"].got[:case.count].tolist() == [3 if int(n) > bound else 0 for n in case.rec_lens]
    assert sum(int(n) <= bound for n in case.rec_lens) >= case.count - 6


@pytest.mark.parametrize("n,count,seq16,length,cid_len", ((1215, 1, True, True, 8), (60, 31, False, False, 0), (63, 32, True, False, 1),
                                                          (1431, 33, False, True, 12), (0, 40, True, True, 0), (2100, 9, True, True, 250)))
def test_parity_uniform_fields(gpu, n, count, seq16, length, cid_len):
    """No per-record array but seq: one length, type and epoch, strides, connection 0."""
    recs = [Rec(rnd(n, f"dtls13 uniform {n} {i}"), BASE - 20 + i, ctype=22, epoch=2) for i in range(count)]
    rl = D.record_len(n, 0, seq16, length, cid_len)
    case = DtlsCase(recs, cid_len=cid_len, seq16=seq16, length=length, expected=BASE, strides=(n + 1 + 3, 5, rl + 7, 3))
    seal_whole(case, uniform=True, where=("uniform", n, count))
    o = open_whole(case, uniform=True, where=("uniform", n, count))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count


PAD_SMALL = (0, 14, 15, 16, 62, 63, 64, 100, 127, 128, 191, 192, 255, 256, 1431, 1791)
PAD_BIG = PAD_SMALL + (2049, 4000, 16127, 16128, 16383, 16384)


@pytest.mark.parametrize("pad_to", (0, 16, 64, 256, 10000))
@pytest.mark.parametrize("which", ("small", "big"))
def test_padding(gpu, which, pad_to):
    """The made bytes -- type byte and zeros -- starting inside a chunk, on a chunk edge and
    spanning whole chunks, in the tail and in whole chunks; with the 16-lane kernel up to the
    cap at 2^14 + 1 (pad_to 256 at 16,384 bytes, pad_to 10,000 at 10,000 bytes and more)."""
    if which == "small" and pad_to == 10000:
        lengths = (0, 1)  # the bound is on the content: these records are 10,000 bytes and more
    else:
        lengths = (PAD_SMALL if which == "small" else PAD_BIG) + ((10000, 9999) if pad_to == 10000 else ())
    case = DtlsCase(parity_records(lengths, f"pad {which} {pad_to}"), cid_len=3, seq16=True, length=True, pad_to=pad_to, expected=BASE)
    assert all(int(v) == D.inner_len(int(n), pad_to) <= D.MAX_INNER for v, n in zip(case.inner, case.lens))
    if pad_to == 10000 and which == "big":
        assert int(case.inner.max()) == D.MAX_INNER and D.inner_len(10000, pad_to) == D.MAX_INNER
    seal_whole(case, max_len=1791 if which == "small" else 16384, where=("pad", which, pad_to))
    o = open_whole(case, max_len=D.MAX_RECORD_LEN if which == "big" or pad_to == 10000 else 2048, where=("pad", which, pad_to))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    assert o.arrays["content_len"].got[:case.count].tolist() == case.lens.tolist()


def test_epoch_rows(gpu):
    """Four epochs of two connections in one batch: seal takes the row from epoch[i], open
    from the wire, and epoch_out says which.  A record sealed under another epoch's keys but
    carrying this epoch's bits fails its tag."""
    recs = [Rec(rnd(40 + 9 * i, f"dtls13 epoch {i}"), BASE + i, kidx=i % 2, ctype=TYPES[i % 6], epoch=(i // 2) % 4 + 4 * (i % 3))
            for i in range(32)]
    case = DtlsCase(recs, cid_len=4, seq16=True, length=True, epoch_rows=True, expected=BASE)
    seal_whole(case, where=("epochs",))
    o = open_whole(case, where=("epochs",))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    assert o.arrays["epoch_out"].got[:case.count].tolist() == [r.epoch % 4 for r in recs]
    # the wrong epoch's keys: the record of epoch e with the bits of e + 1 (no length field, no mask on the first byte)
    msgs = []
    for i in range(case.count):
        m = bytearray(case.protected(i))
        m[0] = (m[0] & ~3) | ((m[0] + 1) & 3)
        msgs.append(bytes(m))
    o = open_whole(case, msgs, where=("wrong epoch",))
    assert o.arrays["status"].got[:case.count].tolist() == [1] * case.count
    assert o.arrays["epoch_out"].got[:case.count].tolist() == [(r.epoch + 1) % 4 for r in recs]


@pytest.mark.parametrize("seq16", (False, True))
def test_sequence_reconstruction(gpu, seq16):
    """The full number from one or two bytes at the window's edges, through `expected`: the
    numbers expected - hwin + 1 .. expected + hwin decode to themselves, the two beyond fail
    their tag, and near zero nothing goes below it."""
    win = 1 << (16 if seq16 else 8)
    h = win // 2
    exp = (5 * win + 77, 3 * win + h, 7)
    offs = (-h - 1, -h, -h + 1, -1, 0, 1, h - 1, h, h + 1)
    recs = [Rec(rnd(33, f"dtls13 window {k} {d}"), exp[k] + d, kidx=k) for k in range(3) for d in offs if exp[k] + d >= 0]
    nb = 2 if seq16 else 1
    decoded = [D.decode_seq(exp[r.kidx], r.seq, nb) for r in recs]
    inside = [d == r.seq for d, r in zip(decoded, recs)]
    assert all(ok for r, ok in zip(recs, inside) if exp[r.kidx] - h < r.seq <= exp[r.kidx] + h) and inside.count(False) >= 4
    case = DtlsCase(recs, seq16=seq16, expected=exp)
    seal_whole(case, where=("window",))
    for keep in (False, True):
        o = open_whole(case, keep=keep, where=("window", keep))
        assert o.arrays["status"].got[:case.count].tolist() == [0 if ok else 1 for ok in inside]
        got = o.arrays["seq_out"].got[:case.count].tolist()
        assert got == [d if ok or keep else 0 for d, ok in zip(decoded, inside)]
    # `expected` moved on by the caller: the same records decode against the new table
    o = open_whole(case, expected=[e + h for e in exp], where=("window moved",))
    moved = [0 if D.decode_seq(exp[r.kidx] + h, r.seq, nb) == r.seq else 1 for r in recs]
    assert o.arrays["status"].got[:case.count].tolist() == moved and moved != [0 if ok else 1 for ok in inside]


def flip(msg: bytes, at: int, mask: int = 0x01) -> bytes:
    m = bytearray(msg)
    m[at] ^= mask
    return bytes(m)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n,max_len", ((0, 2048), (14, 2048), (1431, 2048), (1431, 4096)))
def test_failures(gpu, keep, n, max_len):
    """One bit flipped in every protected field: epoch bits of the first byte, connection ID,
    sequence number bytes, the length field's partner (a record longer by a byte cannot keep
    its length field: that is BAD_HEADER below), first and last ciphertext byte, tag.  All
    fail their tag; the scrub leaves zeros and the sentinels, keep_failed the decryption."""
    cid_len, hl = 5, D.header_len(True, True, 5)
    spots = {"epoch bit": (0, 0x01), "cid first": (1, 0x80), "cid last": (cid_len, 0x01), "seq hi": (1 + cid_len, 0x10),
             "seq lo": (2 + cid_len, 0x01), "ct first": (hl, 0x01), "ct last": (hl + n, 0x80), "tag first": (hl + n + 1, 0x01),
             "tag last": (hl + n + 16, 0x80)}
    recs = [Rec(rnd(n, f"dtls13 fail {n} {i}"), BASE + i, kidx=i % 3, ctype=TYPES[i % 6]) for i in range(len(spots) + 2)]
    case = DtlsCase(recs, cid_len=cid_len, seq16=True, length=True, expected=BASE)
    msgs = [case.protected(i) for i in range(case.count)]
    for i, (at, mask) in enumerate(spots.values()):
        msgs[i + 1] = flip(msgs[i + 1], at, mask)
    o = open_whole(case, msgs, keep=keep, max_len=max_len, where=("failures", n, keep))
    assert o.arrays["status"].got[:case.count].tolist() == [0] + [1] * len(spots) + [0]
    # without the length field a flipped length cannot be told from ciphertext; with it a wrong length is BAD_HEADER
    o = open_whole(case, [flip(m, hl - 1) for m in msgs[:1]] + msgs[1:], keep=keep, max_len=max_len, where=("length field", n))
    assert o.arrays["status"].got[:1].tolist() == [D.BAD_HEADER]


def test_header_short_skipped_no_type(gpu):
    """BAD_HEADER for each of its causes, SHORT, SKIPPED, and NO_TYPE for an all-zero and an
    empty inner plaintext; nothing is written for the first three."""
    cid_len, hl = 2, D.header_len(False, True, 2)
    recs = [Rec(rnd(50, f"dtls13 hdr {i}"), BASE + i, kidx=i % 3) for i in range(12)]
    recs[9] = Rec(b"", BASE + 9, inner=bytes(37))  # authentic and all zero
    recs[10] = Rec(b"", BASE + 10, inner=b"")      # authentic and empty
    recs[11] = Rec(b"", BASE + 11, inner=bytes(64) + b"\x00")
    case = DtlsCase(recs, cid_len=cid_len, length=True, expected=BASE)
    msgs = [case.protected(i) for i in range(case.count)]
    lens = [len(m) for m in msgs]
    msgs[1] = flip(msgs[1], 0, 0x20)   # 000.....
    msgs[2] = flip(msgs[2], 0, 0x80)   # 101.....
    msgs[3] = flip(msgs[3], 0, 0x10)   # C clear with a cid_len
    msgs[4] = flip(msgs[4], hl - 1)    # the length field off by one
    lens[5] = hl + 15                  # no room for a tag
    lens[6] = 0
    lens[7] = 1
    want = [0, 6, 6, 6, 6, 2, 2, 2, 0, 5, 5, 5]
    o = open_whole(case, msgs, lens=lens, max_len=max(lens), where=("header",))
    assert o.arrays["status"].got[:case.count].tolist() == want
    # C set without a cid_len
    plain = DtlsCase(recs[:3], length=True, expected=BASE)
    o = open_whole(plain, [flip(plain.protected(i), 0, 0x10) for i in range(3)], where=("C without cid",))
    assert o.arrays["status"].got[:3].tolist() == [6, 6, 6]
    # longer than max_len: skipped and untouched, seal and open
    o = open_whole(case, max_len=len(case.protected(0)) - 1, where=("skipped",))
    assert o.arrays["status"].got[:case.count].tolist() == [3 if len(case.protected(i)) >= len(case.protected(0)) else s
                                                             for i, s in enumerate([0] * 9 + [5, 5, 5])]
    short = DtlsCase([Rec(rnd(n, f"dtls13 skip {n}"), BASE + n) for n in (10, 11, 12, 11, 0)], expected=BASE)
    seal_whole(short, max_len=11, exp_st=[0, 0, 3, 0, 0], where=("skipped",))


@pytest.mark.parametrize("max_len", (2048, 4096))
def test_strip(gpu, max_len):
    """Contents ending in zero bytes under padding, the type byte on a chunk edge, as the
    tail's only byte and as a chunk's last; zeros running over several rounds of the strip."""
    G = QM.lanes_for(max_len)
    recs = []
    for i, (n, zeros) in enumerate(((63, 3), (64, 5), (65, 64), (127, 0), (128, 1), (64 * G - 1, 7), (64 * G, 9), (64 * G + 1, 1),
                                   (1, 0), (0, 0), (700, 700), (1200, 300), (5, 4), (16 * G, 8 * G), (16 * G + 1, 8 * G + 1))):
        zeros = min(zeros, n)
        recs.append(Rec(rnd(n - zeros, f"dtls13 strip {i}") + bytes(zeros), BASE + i, kidx=i % 3, ctype=TYPES[i % 6]))
    for pad_to in (0, 64, 256):
        case = DtlsCase(recs, seq16=True, pad_to=pad_to, expected=BASE)
        seal_whole(case, max_len=max_len - 300, where=("strip", pad_to))
        o = open_whole(case, max_len=max_len, where=("strip", pad_to))
        assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
        assert o.arrays["content_len"].got[:case.count].tolist() == case.lens.tolist()
        assert o.arrays["type_out"].got[:case.count].tolist() == [r.ctype for r in recs]


def forged_case(cts, seqs, cid_len, kidx):
    """The case whose records carry the given ciphertexts: their inner plaintexts decrypt from them."""
    recs = []
    for ct, seq in zip(cts, seqs):
        key, iv = KEYS[32 * kidx:32 * kidx + 32], IVS[12 * kidx:12 * kidx + 12]
        recs.append(Rec(b"", seq, kidx=kidx, inner=R.xor_stream(key, D.nonce_of(iv, seq), ct)))
    return DtlsCase(recs, cid_len=cid_len, seq16=cid_len != 0, length=cid_len != 0, expected=seqs[0])


def header_for(case: DtlsCase, kidx: int, seq: int, n: int) -> bytes:
    c = min(kidx, case.num_conns - 1)
    return D.header_of(case.seq16, case.length, case.cids[case.cid_len * c:case.cid_len * (c + 1)], 0, seq, n + 16)


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("cid_len", (0, 12))
def test_mac_finish_edges(gpu, max_len, cid_len):
    """Records whose ciphertext drives the Poly1305 accumulator to mac_forge.TARGETS (p - 1 ..
    p - 5, 2^128 -+, 2^129, the all-zero and all-ones tags) behind the 2-byte
    (the minimal header) and the 17-byte header, at a 1,200-byte and a 64-byte
    ciphertext, opened by the 8-lane and the 16-lane kernel: status 0 or 5 as the reference
    says and its plaintext; and sealed again from the decrypted content where it ends in a type."""
    kidx, cts, seqs = 1, [], []
    shape = DtlsCase([], cid_len=cid_len, seq16=cid_len != 0, length=cid_len != 0)
    key, iv = KEYS[32:64], IVS[12:24]
    for n in (1200, 64):
        for name, T in mf.TARGETS.items():
            seq = 2**33 + 4000 + len(cts)
            nonce, ad = D.nonce_of(iv, seq), header_for(shape, kidx, seq, n)
            assert len(ad) == (17 if cid_len else 2)
            r, s = RB.poly_rs(key, nonce)
            target = (T(r, s, None) if callable(T) else T) % RB.P
            ct, _ = RB.forge_ct(key, nonce, ad, n, target, f"dtls13 {name} {n} {cid_len}")
            assert RB.accumulator(key, nonce, ad, ct) == target
            if name in mf.TAG_PATTERN:
                assert R.tag_of(key, nonce, ad, ct) == mf.TAG_PATTERN[name]
            assert QM.tag(key, nonce, ad, ct, QM.lanes_for(max_len)) == R.tag_of(key, nonce, ad, ct)
            cts.append(ct)
            seqs.append(seq)
    case = forged_case(cts, seqs, cid_len, kidx)
    for i, ct in enumerate(cts):
        assert case.protected(i)[case.hdr_len:-16] == ct
    o = open_whole(case, max_len=max_len, where=("finish", max_len, cid_len))
    assert all(s in (0, 5) for s in o.arrays["status"].got[:case.count].tolist())
    sealable = [Rec(r.inner[:-1], r.seq, kidx=kidx, ctype=r.inner[-1]) for r in case.recs if r.inner[-1]]
    assert len(sealable) > case.count // 2
    again = DtlsCase(sealable, cid_len=cid_len, seq16=cid_len != 0, length=cid_len != 0, expected=seqs[0])
    seal_whole(again, max_len=max_len - 300, where=("finish", max_len, cid_len))


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("cid_len", (0, 12))
@pytest.mark.parametrize("tname", ("m1", "zero"))
def test_mac_lane_sums(gpu, max_len, cid_len, tname):
    """Every per-lane sum of the kernel's MAC, and the tail slot's, forged to p - 1 (all limbs
    at their maximum) and to 0, behind a one-block and a two-block header.  A lane that holds
    the additional data alone cannot be steered: forge_lanes reports it."""
    G = QM.lanes_for(max_len)
    kidx, cts, seqs = 2, [], []
    shape = DtlsCase([], cid_len=cid_len, seq16=cid_len != 0, length=cid_len != 0)
    key, iv = KEYS[64:96], IVS[24:36]
    for k, n in enumerate((1252, 100, 64 * (G + 3) + 52, 64 * G + 36)):
        seq = 2**34 + 9000 + k
        nonce, ad = D.nonce_of(iv, seq), header_for(shape, kidx, seq, n)
        ct, tries, skipped = QS.forge_lanes(key, nonce, ad, n, G, mf.B_TARGETS[tname], f"dtls13 {tname} {n} {G} {cid_len}")
        r, _ = RB.poly_rs(key, nonce)
        H, ts = QM.lane_sums(R.mac_stream(ad, ct), len(ad), n, r, G)
        sets = QM.lane_sets(len(ad), n, G)[:-1]
        alone = [t for t, blocks in sets if all(b < (len(ad) + 15) // 16 for b in blocks)]
        assert skipped == len(alone)
        assert ts == mf.B_TARGETS[tname] and all(H[t] == mf.B_TARGETS[tname] for t, _ in sets if t not in alone)
        assert QM.tag(key, nonce, ad, ct, G) == R.tag_of(key, nonce, ad, ct)
        cts.append(ct)
        seqs.append(seq)
    case = forged_case(cts, seqs, cid_len, kidx)
    for i, ct in enumerate(cts):
        assert case.protected(i)[case.hdr_len:-16] == ct
    o = open_whole(case, max_len=max_len, where=("lanes", max_len, cid_len, tname))
    assert all(s in (0, 5) for s in o.arrays["status"].got[:case.count].tolist())
    sealable = [Rec(r.inner[:-1], r.seq, kidx=kidx, ctype=r.inner[-1]) for r in case.recs if r.inner[-1]]
    if sealable:
        again = DtlsCase(sealable, cid_len=cid_len, seq16=cid_len != 0, length=cid_len != 0, expected=seqs[0])
        seal_whole(again, max_len=max_len - 300, where=("lanes", max_len, cid_len, tname))


def test_graph_capture(gpu):
    """One seal and one open captured on a single stream, a linear chain, and replayed once:
    the bytes of the direct calls."""
    import torch

    from suruga_amd import dtls13 as DT

    count = 48
    recs = [Rec(rnd(1200 - i % 7, f"dtls13 graph {i}"), BASE - 20 + i, kidx=i % 3, ctype=TYPES[i % 6], epoch=i % 4) for i in range(count)]
    case = DtlsCase(recs, cid_len=8, seq16=True, length=True, pad_to=16, expected=BASE)
    inp = torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda")
    for o, r in zip(case.raw_off, recs):
        inp[int(o):int(o) + len(r.content)] = dev_bytes(r.content)
    tables = dict(keys=dev_bytes(case.keys), ivs=dev_bytes(case.ivs), sn_keys=dev_bytes(case.sns), cid_len=8,
                  key_index=dev_u32([r.kidx for r in recs]))
    seq, types, epochs = (dev_u64([r.seq for r in recs]), dev_u8(np.array([r.ctype for r in recs], dtype=np.uint8)),
                          dev_u8(np.array([r.epoch for r in recs], dtype=np.uint8)))
    cids, expected = dev_bytes(case.cids), dev_u64(case.expected)
    lens, rlens = dev_u32(case.lens), dev_u32(case.rec_lens)
    raw_off, rec_off = dev_u64(case.raw_off), dev_u64(case.rec_off)

    def run(ct, back, st, seq_out, ep_out, clen, ty_out, stream):
        DT.seal_dtls13(DT.Dtls13Batch(count=count, inp=inp, out=ct, status=st[:count], lens=lens, max_len=1300, in_off=raw_off,
                                      out_off=rec_off, seq=seq, type=types, epoch=epochs, cids=cids, pad_to=16, seq16=True,
                                      length=True, stream=stream, **tables))
        DT.open_dtls13(DT.Dtls13Batch(count=count, inp=ct, out=back, status=st[count:], seq_out=seq_out, epoch_out=ep_out,
                                      content_len=clen, type_out=ty_out, expected=expected, lens=rlens, max_len=1400,
                                      in_off=rec_off, out_off=raw_off, stream=stream, **tables))

    def buffers():
        return (torch.zeros(case.rec_size + 16, dtype=torch.uint8, device="cuda"),
                torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda"), filled(2 * count, 0xFF),
                torch.full((count,), -1, dtype=torch.int64, device="cuda"), filled(count, 0xEE),
                torch.full((count,), -1, dtype=torch.int32, device="cuda"), filled(count, 0xEE))

    fills = (0, 0, 0xFF, -1, 0xEE, -1, 0xEE)
    direct, captured = buffers(), buffers()
    run(*direct, None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(*captured, torch.cuda.current_stream())
    for t, v in zip(captured, fills):
        t.fill_(v)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(direct, captured):
        assert bool(torch.equal(a, b))
    ct_h, back_h = host_bytes(direct[0]), host_bytes(direct[1])
    assert host_bytes(direct[2]) == bytes(2 * count)
    assert host_np(direct[3]).view(np.uint64).tolist() == [r.seq for r in recs]
    assert host_np(direct[4]).tolist() == [r.epoch for r in recs]
    assert host_np(direct[5]).tolist() == case.lens.tolist()
    assert host_np(direct[6]).tolist() == [r.ctype for r in recs]
    for i in range(count):
        lo = int(case.rec_off[i])
        assert ct_h[lo:lo + len(case.protected(i))] == case.protected(i)
        lo = int(case.raw_off[i])
        assert back_h[lo:lo + len(recs[i].content)] == recs[i].content


def test_round_trip_zipf(gpu):
    """dtls13.py end to end: a few hundred contents of Zipf lengths over 5 connections with keys
    from record_keys through seal and two opens, `expected` advanced between them; sequence
    numbers, lengths, types and contents come back, and a few records are the reference's."""
    import torch

    import suruga_amd as S
    from suruga_amd import workloads as WL

    count, conns, cid_len = 384, 5, 6
    k = WL.zipf_lengths(count) // 64
    lens = np.clip(64 * k - 63 + (13 * np.arange(count)) % 64, 0, 16384).astype(np.uint32)
    rlens = np.array([D.record_len(int(n), 64, True, True, cid_len) for n in lens], dtype=np.uint32)
    assert all(S.dtls13_record_len(int(n), 64, True, True, cid_len) == int(m) for n, m in zip(lens[:64], rlens[:64]))
    slot = (rlens.astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(16)
    rec_off = np.concatenate(([0], np.cumsum(slot)[:-1])).astype(np.uint64) + (np.arange(count, dtype=np.uint64) % np.uint64(16))
    size = int(rec_off[-1] + slot[-1]) + 16
    host = np.random.default_rng(9147).integers(1, 256, size=size, dtype=np.uint8)  # no zero byte: the content's length is exact
    secrets = np.frombuffer(R.data(32 * conns, b"dtls13 zipf secrets"), dtype=np.uint8).reshape(conns, 32)
    keys, ivs, sns = S.dtls13_record_keys(secrets)
    assert (keys[3].tobytes(), ivs[3].tobytes(), sns[3].tobytes()) == D.record_keys(secrets[3].tobytes())
    cids = R.data(cid_len * conns, b"dtls13 zipf cids")
    kidx = np.arange(count) % conns
    half = count // 2
    # each connection's numbers run on from just below a multiple of 2^16, 400 apart: either half of the batch
    # stays within 2^15 of its expected number, the whole batch does not
    base = [(j + 1) * 2**16 - 20 for j in range(conns)]
    seqs = [base[int(kidx[i])] + (i // conns) * 400 for i in range(count)]
    types = (np.arange(count) * 7 % 255 + 1).astype(np.uint8)
    src, ct = torch.from_numpy(host.copy()).to("cuda"), torch.zeros(size, dtype=torch.uint8, device="cuda")
    back = torch.zeros(size, dtype=torch.uint8, device="cuda")
    st = filled(count, 0xFF)
    tables = dict(keys=dev_bytes(keys.tobytes()), ivs=dev_bytes(ivs.tobytes()), sn_keys=dev_bytes(sns.tobytes()), cid_len=cid_len)
    S.seal_dtls13(S.Dtls13Batch(count=count, inp=src, out=ct, status=st, seq=dev_u64(seqs), type=dev_u8(types), uniform_epoch=3,
                                cids=dev_bytes(cids), pad_to=64, seq16=True, length=True, lens=dev_u32(lens), max_len=16384,
                                in_off=dev_u64(rec_off), out_off=dev_u64(rec_off), key_index=dev_u32(kidx), **tables))
    torch.cuda.synchronize()
    assert host_bytes(st) == bytes(count)
    sealed = host_np(ct)
    for i in (0, 1, 77, int(np.argmax(lens)), int(np.argmin(lens)), count - 1):
        o, n, j = int(rec_off[i]), int(lens[i]), int(kidx[i])
        want = D.protect(keys[j].tobytes(), ivs[j].tobytes(), sns[j].tobytes(), seqs[i], host[o:o + n].tobytes(), int(types[i]),
                         pad_to=64, epoch=3, cid=cids[cid_len * j:cid_len * (j + 1)], seq16=True, length=True)
        assert sealed[o:o + int(rlens[i])].tobytes() == want, i
    got_seq, got_len, got_type = [], [], []
    for lo, hi in ((0, half), (half, count)):
        # the caller's part: expected is the highest number seen so far + 1 (the first call: the first number)
        expected = [max([seqs[i] + 1 for i in range(lo) if kidx[i] == j], default=base[j]) for j in range(conns)]
        n = hi - lo
        seq_out, ep_out, clen, ty_out = dev_u64([0] * n), filled(n, 0xEE), dev_u32([0] * n), filled(n, 0xEE)
        st = filled(n, 0xFF)
        S.open_dtls13(S.Dtls13Batch(count=n, inp=ct, out=back, status=st, seq_out=seq_out, epoch_out=ep_out, content_len=clen,
                                    type_out=ty_out, expected=dev_u64(expected), lens=dev_u32(rlens[lo:hi]),
                                    max_len=D.MAX_RECORD_LEN, in_off=dev_u64(rec_off[lo:hi]), out_off=dev_u64(rec_off[lo:hi]),
                                    key_index=dev_u32(kidx[lo:hi]), **tables))
        torch.cuda.synchronize()
        assert host_bytes(st) == bytes(n) and host_bytes(ep_out) == bytes([3]) * n
        got_seq += host_np(seq_out).view(np.uint64).tolist()
        got_len += host_np(clen).view(np.uint32).tolist()
        got_type += host_np(ty_out).tolist()
    assert got_seq == seqs and got_len == lens.tolist() and got_type == types.tolist()
    plain = host_np(back)
    for i in range(count):
        o, n = int(rec_off[i]), int(lens[i])
        assert np.array_equal(plain[o:o + n], host[o:o + n]), i
