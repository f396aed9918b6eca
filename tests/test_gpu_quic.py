"""sg_seal_batch_quic / sg_open_batch_quic (sg_quic.hip) on the GPU against tests/quic_ref.py.

Every data buffer sits in a footprint.sentinel buffer with a margin in front and behind and
is compared whole afterwards, with the status bytes and pn_out, so a byte written outside a
packet's own output fails as a wrong byte inside it does (tests/quic_support.py).  All
comparisons are byte equality.  The kernel runs with 8 lanes a packet where the call's
max_len is at most 2 KiB and with 16 otherwise; the cases that matter to both say so."""
from __future__ import annotations

import numpy as np
import pytest

import mac_forge as mf
import quic_model as QM
import quic_ref as Q
import rfc8439_ref as R
import rfc_batch_support as RB
from gpu_support import dev_bytes, dev_u32, dev_u64, filled, host_bytes, host_np
from quic_support import (HPS3, IVS3, KEYS3, M, PN_EDGES, PN_OFFS, Pkt, QuicCase, forge_lanes, long_, open_whole, rnd, seal_whole,
                          short)

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 3, 15, 16, 17, 47, 48, 63, 64, 65, 1162, 1431)
PN_LEN_OF = {0: 4, 1: 3, 3: 1}  # the shortest packets that still hold a sample
LONGEST = 16384 - 16 - 255      # payload of the longest packet: pn_off 251, pn_len 4


def parity_packets(lengths, extra=0):
    """Every length with every pn_len it allows, the packet number offsets, packet numbers and
    connections taken in turn (connection 5 lies beyond the 3-row tables: clamped), one packet
    in four with a long header; `extra` more of drawn lengths up to 1,500 bytes."""
    pkts = []
    for idx, n in enumerate(lengths):
        for j in range(4):
            i = len(pkts)
            pn_len = PN_LEN_OF.get(n, j + 1)
            b0 = long_(pn_len) if j == 2 else short(pn_len, phase=i & 1)
            pkts.append(Pkt(b0, PN_OFFS[(idx + j) % 4], PN_EDGES[(idx // 4 + j) % 4], rnd(n, f"pl {n} {j}"),
                            kidx=(0, 1, 2, 5)[(i // 2) % 4], tag=str(i)))
    draw = np.random.default_rng(9001).integers(0, 1501, size=extra)
    for k, n in enumerate(draw.tolist()):
        i = len(pkts)
        pn_len = 4 if n < 3 else 1 + k % 4
        pkts.append(Pkt(short(pn_len), PN_OFFS[k % 3], 7 * i + (k << 20), rnd(n, f"extra {k}"), kidx=k % 3, tag=str(i)))
    return pkts


_cases: dict = {}


def parity_case(which: str) -> QuicCase:
    """"big": every length and the longest (16 lanes a packet); "small": every length but the
    longest and 280 drawn ones, 332 packets (8 lanes: eleven workgroups, the last ragged)."""
    if which not in _cases:
        if which == "big":
            pkts = parity_packets(LENGTHS) + [Pkt(short(4), 251, 2**62 - 1, rnd(LONGEST, "longest"), kidx=2, tag="L")]
        else:
            pkts = parity_packets(LENGTHS, extra=280)
        _cases[which] = QuicCase(pkts)
    return _cases[which]


def test_rfc9001_a5(gpu):
    """Seal gives appendix A.5's packet byte for byte; open returns it from any expected
    number of the window."""
    a = Q.A5
    mk = lambda exp: Pkt(0x42, 1, a["pn"], a["payload"], exp=exp)  # noqa: E731
    case = QuicCase([mk(None), mk(a["pn"] - 2**23), mk(a["pn"] + 2**23 - 1)], keys=a["key"], ivs=a["iv"], hps=a["hp"])
    assert case.pkts[0].header() == a["header"] and case.protected(0) == a["packet"]
    o = seal_whole(case, where=("A.5",))
    lo = int(case.prot_off[0]) + M
    assert o.out[lo:lo + 21].tobytes() == a["packet"]
    o = open_whole(case, where=("A.5",))
    lo = int(case.raw_off[1]) + M
    assert o.out[lo:lo + 5].tobytes() == a["header"] + a["payload"]
    assert o.arrays["pn_out"].got[:3].tolist() == [a["pn"]] * 3


@pytest.mark.parametrize("which", ("big", "small"))
def test_parity_per_packet_arrays(gpu, which):
    """Seal and open of every length, pn_len, pn_off, header form, skew pair, packet number
    edge and connection in one batch, whole buffers."""
    case = parity_case(which)
    assert QM.lanes_for(int(case.raw_lens.max()) + 16) == (16 if which == "big" else 8)
    skews = {(int(a) % 16, int(b) % 16) for a, b in zip(case.raw_off, case.prot_off)}
    assert len(skews) == (256 if which == "small" else case.count)  # input and output skews 0..15, independently
    seal_whole(case, where=(which,))
    open_whole(case, where=(which,))


@pytest.mark.parametrize("n,count", ((1215, 40), (60, 33)))
def test_parity_uniform_fields(gpu, n, count):
    """No per-packet array at all: uniform_len, uniform_pn_off, strides, connection 0."""
    pkts = [Pkt(short(2), 9, 2**32 - 3 + i, rnd(n, f"uni {i}"), tag="u") for i in range(count)]
    case = QuicCase(pkts, strides=(n + 11 + 5, 3, n + 11 + 16 + 3, 1))  # odd strides from odd bases
    seal_whole(case, uniform=True, where=("uniform", n))
    open_whole(case, uniform=True, where=("uniform", n))


def test_key_phase(gpu):
    """Two generations a connection, packets of both phases and long-header packets in one
    batch: rows 2 k + phase, long headers row 2 k; without the flag a phase 1 packet fails."""
    keys = b"".join(R.data(32, b"kp key %d" % i) for i in range(4))
    ivs = b"".join(R.data(12, b"kp iv %d" % i) for i in range(4))
    hps = HPS3[:64]
    pkts = []
    for i in range(24):
        b0 = long_(1 + i % 4) | 0x04 if i % 3 == 2 else short(1 + i % 4, phase=(i >> 1) & 1)  # 0x04 in a long header is no phase
        pkts.append(Pkt(b0, PN_OFFS[i % 4], 1000 + i, rnd(30 + 50 * i, f"kp {i}"), kidx=(0, 1, 7)[i % 3], tag=f"kp{i}"))
    case = QuicCase(pkts, keys=keys, ivs=ivs, hps=hps, key_phase=True)
    seal_whole(case, where=("key phase",))
    open_whole(case, where=("key phase",))
    # the same packets through tables without the flag: rows k, so connection 0 under phase 0 (row 0) still opens,
    # and everything sealed under a row 2 k + 1 or for connection 1 (row 2, read as row 1) fails
    flat = QuicCase(pkts, keys=keys[:64], ivs=ivs[:24], hps=hps, key_phase=False)
    prot = [case.protected(i) for i in range(case.count)]
    o = open_whole(flat, prot, where=("no flag",))
    st = o.arrays["status"].got[:24].tolist()
    for i, p in enumerate(pkts):
        phase = 0 if p.b0 & 0x80 else (p.b0 >> 2) & 1
        assert st[i] == (0 if case.conn(i) == 0 and phase == 0 else 1), (i, st[i])
    assert 0 in st and 1 in st


def test_packet_number_decode(gpu):
    """Packets sealed with numbers at and just beyond each edge of the window of the given
    expected number: inside it opens with the number; one beyond decodes a window away, so
    the nonce is another and the tag fails."""
    pkts, inside = [], []
    for pn_len in (1, 2, 3, 4):
        half = 1 << (8 * pn_len - 1)
        for exp in (5 * half + 3, 2**40 + 1, half - 1, 2**62 - 1):
            for d in (-half, -half + 1, 0, half, half + 1):
                pn = exp + d
                if not 0 <= pn < 2**62:
                    continue
                pkts.append(Pkt(short(pn_len), 9, pn, rnd(40, f"dec {pn_len} {exp} {d}"), exp=exp, tag="d"))
                inside.append(Q.decode_pn(exp, pn % (2 * half), pn_len) == pn)
                # one beyond either edge is a window away, unless 0 or 2^62 is in the way
                assert inside[-1] == (-half < d <= half) or exp in (half - 1, 2**62 - 1)
    case = QuicCase(pkts)
    o = open_whole(case, where=("decode",))
    st = o.arrays["status"].got[:case.count].tolist()
    assert st == [0 if ok else 1 for ok in inside]
    assert inside.count(False) >= 12 and inside.count(True) >= 36


def flip(pkt: bytes, at: int, mask: int = 0x01) -> bytes:
    b = bytearray(pkt)
    b[at] ^= mask
    return bytes(b)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n", (100, 1300, 2500))
def test_failures(gpu, keep, n):
    """A flipped bit in the protected first byte (pn_len bits and the key phase bit), a packet
    number byte, the sample, the ciphertext behind it and the tag: SG_E_BAD_MAC, the output
    all zero and pn_out 0 -- or with SG_QUIC_KEEP_FAILED what the reference decrypts -- and the
    good packets between them untouched.  A packet of pn_off + 19 bytes is too short."""
    pn_off, pn_len = 9, 2
    hdr = pn_off + pn_len
    flips = [(0, 0x01), (0, 0x02), (0, 0x04), (0, 0x80), (pn_off, 0x10), (pn_off + 1, 0x01), (pn_off + 4, 0x01), (pn_off + 19, 0x80),
             (hdr + n // 2, 0x01), (hdr + n - 1, 0x40), (hdr + n, 0x01), (hdr + n + 15, 0x80)]
    pkts = [Pkt(short(pn_len), pn_off, 77000 + i, rnd(n, f"fail {n} {i}"), kidx=i % 3, tag=f"f{i}") for i in range(2 * len(flips) + 2)]
    case = QuicCase(pkts)
    prot = [case.protected(i) for i in range(case.count)]
    want_bad = []
    for k, (at, mask) in enumerate(flips):
        prot[2 * k + 1] = flip(prot[2 * k + 1], at, mask)
        want_bad.append(2 * k + 1)
    lens = [len(p) for p in prot]
    lens[-1] = pn_off + 19  # one byte short of a sample
    o = open_whole(case, prot, lens=lens, keep=keep, where=("failures", n, keep))
    st = o.arrays["status"].got[:case.count].tolist()
    assert st == [1 if i in want_bad else 0 for i in range(case.count - 1)] + [2]


def test_short_and_skipped(gpu):
    """Seal: pn_len + payload = 3 is SG_E_SHORT (no full sample), 4 is sealed; a packet of
    max_len + 1 bytes is SG_STATUS_SKIPPED in both directions, nothing of it touched, and the
    call returns SG_OK.  A per-packet pn_off of 0 or 252 is SG_E_SHORT."""
    pkts = [Pkt(short(1), 9, 5, rnd(2, "s0")), Pkt(short(1), 9, 6, rnd(3, "s1")), Pkt(short(2), 1, 7, rnd(1, "s2")),
            Pkt(short(3), 21, 8, b""), Pkt(short(4), 9, 9, b""), Pkt(short(2), 9, 10, rnd(300, "s5")),
            Pkt(short(2), 9, 11, rnd(301, "s6")), Pkt(short(2), 9, 12, rnd(200, "s7"))]
    case = QuicCase(pkts)
    max_len = 9 + 2 + 300
    want = [2, 0, 2, 2, 0, 0, 3, 0]
    seal_whole(case, max_len=max_len, exp_st=want, where=("short",))
    # open: the sealed ones, with max_len one below the longest
    # (what a seal refuses is, with 16 bytes more, shorter than pn_off + 20 as well: zeros stand in for it)
    prot = [case.protected(i) if want[i] != 2 else bytes(int(case.raw_lens[i]) + 16) for i in range(case.count)]
    o = open_whole(case, prot, max_len=max_len + 16, exp={6: (3, None, None)}, where=("skipped",))
    assert o.arrays["status"].got[:8].tolist() == want
    # per packet: a pn_off outside 1..251, one beyond the packet (100) and one whose header ends beyond it (60)
    bad = QuicCase([Pkt(short(2), 9, i + 1, rnd(50, f"b{i}")) for i in range(5)])
    from suruga_amd import quic as QU

    out, st = filled(4096, 0x5A), filled(5, 0xFF)
    inp = dev_bytes(b"".join(p.raw().ljust(128, b"\0") for p in bad.pkts))
    args = dict(count=5, keys=dev_bytes(KEYS3), ivs=dev_bytes(IVS3), hp_keys=dev_bytes(HPS3), pn=dev_u64([1, 2, 3, 4, 5]),
                pn_out=dev_u64([9] * 5), pn_off=dev_u32([0, 9, 252, 100, 60]), uniform_len=61, in_stride=128,
                out_stride=256, inp=inp, out=out, status=st)
    QU.seal_quic(QU.QuicBatch(**args))
    assert host_bytes(st) == bytes([2, 0, 2, 2, 2])
    got = host_np(out)
    assert got[256:256 + 77].tobytes() == bad.protected(1) and (got[:256] == 0x5A).all() and (got[256 + 77:] == 0x5A).all()
    st.fill_(0xFF)
    QU.open_quic(QU.QuicBatch(**dict(args, uniform_len=77)))
    assert [host_bytes(st)[i] for i in (0, 2, 3, 4)] == [2, 2, 2, 2]


def forged_packet(key, iv, hp, pn, header, ct, pn_off):
    """The protected packet of a chosen ciphertext: its tag by the sequential reference."""
    nonce = Q.nonce_of(iv, pn)
    return Q.apply_hp(hp, header + ct + R.tag_of(key, nonce, header, ct), pn_off)


@pytest.mark.parametrize("max_len", (2048, 4096))
def test_mac_finish_edges(gpu, max_len):
    """Packets whose ciphertext drives the Poly1305 accumulator to mac_forge.TARGETS (p - 1 ..
    p - 5, 2^128 -+, 2^129, the all-zero and all-ones tags), at a 1,200-byte and a 64-byte
    payload, opened by the 8-lane (max_len 2048) and the 16-lane kernel: status 0 and the
    reference's plaintext."""
    key, iv, hp = KEYS3[:32], IVS3[:12], HPS3[:32]
    pkts, prot, names = [], [], []
    for n in (1200, 64):
        for name, T in mf.TARGETS.items():
            pn = 4000 + len(pkts)
            nonce = Q.nonce_of(iv, pn)
            p = Pkt(short(2), 9, pn, b"", tag="m")
            header = Q.header_of(p.raw(), 9, pn)
            r, s = RB.poly_rs(key, nonce)
            target = (T(r, s, None) if callable(T) else T) % RB.P
            ct, _ = RB.forge_ct(key, nonce, header, n, target, f"quic {name} {n}")
            assert RB.accumulator(key, nonce, header, ct) == target
            tag = R.tag_of(key, nonce, header, ct)
            if name in mf.TAG_PATTERN:
                assert tag == mf.TAG_PATTERN[name]
            p.payload = R.xor_stream(key, nonce, ct)
            pkts.append(p)
            prot.append(forged_packet(key, iv, hp, pn, header, ct, 9))
            names.append(name)
    case = QuicCase(pkts)
    assert [case.protected(i) for i in range(case.count)] == prot  # the forged ciphertext is what sealing its plaintext gives
    o = open_whole(case, prot, max_len=max_len, where=("finish", max_len))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    seal_whole(case, max_len=max_len - 16, where=("finish", max_len))


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("tname", ("m1", "zero"))
def test_mac_lane_sums(gpu, max_len, tname):
    """Every per-lane sum of the kernel's MAC, and the tail slot's, forged to p - 1 (all limbs
    at their maximum) and to 0, as Tier B does for the packed kernel."""
    G = QM.lanes_for(max_len)
    key, iv, hp = KEYS3[32:64], IVS3[12:24], HPS3[32:64]
    pkts, prot = [], []
    for k, n in enumerate((1248, 96, 64 * (G + 3) + 48)):
        pn = 9000 + k
        nonce = Q.nonce_of(iv, pn)
        p = Pkt(short(3), 21, pn, b"", kidx=1, tag="l")
        header = Q.header_of(p.raw(), 21, pn)
        ct, tries, skipped = forge_lanes(key, nonce, header, n, G, mf.B_TARGETS[tname], f"{tname} {n} {G}")
        assert skipped <= 1
        r, _ = RB.poly_rs(key, nonce)
        H, ts = QM.lane_sums(R.mac_stream(header, ct), len(header), n, r, G)
        na = (len(header) + 15) // 16
        steered = [t for t, blocks in QM.lane_sets(len(header), n, G)[:-1] if blocks[-1] >= na]
        assert ts == mf.B_TARGETS[tname] and all(H[t] == mf.B_TARGETS[tname] for t in steered)
        assert len(steered) == -(-(n // 64) // QM.geom(n, G)[1])
        assert QM.tag(key, nonce, header, ct, G) == R.tag_of(key, nonce, header, ct)
        p.payload = R.xor_stream(key, nonce, ct)
        pkts.append(p)
        prot.append(forged_packet(key, iv, hp, pn, header, ct, 21))
    case = QuicCase(pkts)
    o = open_whole(case, prot, max_len=max_len, where=("lanes", max_len, tname))
    assert o.arrays["status"].got[:3].tolist() == [0, 0, 0]
    seal_whole(case, max_len=max_len - 16, where=("lanes", max_len, tname))


def test_graph_capture(gpu):
    """One seal and one open captured on a single stream and replayed once: the bytes of the
    direct calls."""
    import torch

    from suruga_amd import quic as QU

    count, n, pn_off = 300, 1200, 9
    pkts = [Pkt(short(1 + i % 4), pn_off, 50000 + 3 * i, rnd(n - i % 7, f"cap {i}"), kidx=i % 3, tag="c") for i in range(count)]
    case = QuicCase(pkts)
    inp = torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda")
    for o, p in zip(case.raw_off, pkts):
        inp[int(o):int(o) + len(p.raw())] = dev_bytes(p.raw())
    tables = dict(keys=dev_bytes(KEYS3), ivs=dev_bytes(IVS3), hp_keys=dev_bytes(HPS3), key_index=dev_u32([p.kidx for p in pkts]),
                  pn_off=dev_u32([pn_off] * count), pn=dev_u64([p.pn for p in pkts]))
    lens, plens = dev_u32(case.raw_lens), dev_u32(case.raw_lens + 16)
    raw_off, prot_off = dev_u64(case.raw_off), dev_u64(case.prot_off)

    def run(ct, back, st, pn_out, stream):
        QU.seal_quic(QU.QuicBatch(count=count, inp=inp, out=ct, status=st[:count], lens=lens, max_len=1300, in_off=raw_off,
                                  out_off=prot_off, stream=stream, **tables))
        QU.open_quic(QU.QuicBatch(count=count, inp=ct, out=back, status=st[count:], pn_out=pn_out, lens=plens, max_len=1300,
                                  in_off=prot_off, out_off=raw_off, stream=stream, **tables))

    def buffers():
        return (torch.zeros(case.prot_size + 16, dtype=torch.uint8, device="cuda"),
                torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda"), filled(2 * count, 0xFF),
                torch.full((count,), -1, dtype=torch.int64, device="cuda"))

    direct, captured = buffers(), buffers()
    run(*direct, None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(*captured, torch.cuda.current_stream())
    for t in captured[:2]:
        t.zero_()
    captured[2].fill_(0xFF)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(direct, captured):
        assert bool(torch.equal(a, b))
    ct_h, back_h = host_bytes(direct[0]), host_bytes(direct[1])
    assert host_bytes(direct[2]) == bytes(2 * count)
    assert host_np(direct[3]).tolist() == [p.pn for p in pkts]
    for i in range(0, count, 13):
        lo = int(case.prot_off[i])
        assert ct_h[lo:lo + len(case.protected(i))] == case.protected(i)
        lo = int(case.raw_off[i])
        assert back_h[lo:lo + len(pkts[i].raw())] == pkts[i].header() + pkts[i].payload


def test_round_trip_with_derived_keys(gpu):
    """quic.py end to end with the tables of quic_packet_keys: seal and open under the first
    generation, then after update=1 under the second (the header protection keys stay)."""
    import torch

    import suruga_amd as S

    conns, count, n, pn_off = 5, 200, 1250, 9
    secrets = np.frombuffer(b"".join(R.data(32, b"quic secret %d" % i) for i in range(conns)), dtype=np.uint8).reshape(conns, 32)
    keys, ivs, hps = S.quic_packet_keys(secrets, threads=2)
    assert (keys[3].tobytes(), ivs[3].tobytes(), hps[3].tobytes()) == Q.packet_keys(secrets[3].tobytes())
    payload = [rnd(n, f"rt {i}") for i in range(count)]
    stride_in, stride_out = pn_off + 2 + n + 3, pn_off + 2 + n + 16 + 1
    raw = b"".join((bytes([0x41]) + bytes(pn_off - 1) + b"\0\0" + p).ljust(stride_in, b"\0") for p in payload)
    kidx = dev_u32([i % conns for i in range(count)])
    hp_d = dev_bytes(hps.tobytes())
    for gen in range(2):
        if gen:
            keys, ivs, secrets = S.quic_packet_keys(secrets, update=True)
            assert keys[2].tobytes() == Q.packet_keys(Q.next_secret(R.data(32, b"quic secret 2")))[0]
        tables = dict(keys=dev_bytes(keys.tobytes()), ivs=dev_bytes(ivs.tobytes()), hp_keys=hp_d, key_index=kidx,
                      uniform_pn_off=pn_off)
        ct = torch.zeros(count * stride_out, dtype=torch.uint8, device="cuda")
        back = torch.zeros(count * stride_in, dtype=torch.uint8, device="cuda")
        st, pn_out = filled(count, 0xFF), dev_u64([0] * count)
        pns = [2**32 - 100 + i + 1000 * gen for i in range(count)]
        S.seal_quic(S.QuicBatch(count=count, inp=dev_bytes(raw), out=ct, status=st, pn=dev_u64(pns), uniform_len=pn_off + 2 + n,
                                in_stride=stride_in, out_stride=stride_out, **tables))
        torch.cuda.synchronize()
        assert host_bytes(st) == bytes(count)
        k, v, h = keys[7 % conns].tobytes(), ivs[7 % conns].tobytes(), hps[7 % conns].tobytes()
        assert host_bytes(ct)[7 * stride_out:8 * stride_out - 1] == Q.protect(k, v, h, pns[7], raw[7 * stride_in:8 * stride_in - 3], pn_off)
        st.fill_(0xFF)
        S.open_quic(S.QuicBatch(count=count, inp=ct, out=back, status=st, pn=dev_u64([p - 50 for p in pns]), pn_out=pn_out,
                                uniform_len=pn_off + 2 + n + 16, in_stride=stride_out, out_stride=stride_in, **tables))
        torch.cuda.synchronize()
        assert host_bytes(st) == bytes(count) and host_np(pn_out).tolist() == pns
        back_h = host_bytes(back)
        for i in range(count):
            got = back_h[i * stride_in:i * stride_in + pn_off + 2 + n]
            assert got[pn_off + 2:] == payload[i] and got[pn_off:pn_off + 2] == (pns[i] & 0xFFFF).to_bytes(2, "big"), i
