"""sg_seal_batch_wg / sg_open_batch_wg (sg_wg.hip) on the GPU against tests/wg_ref.py.

Every data buffer sits in a footprint.sentinel buffer with a margin in front and behind and
is compared whole afterwards, with the status bytes, counter_out and inner_len, so a byte
written outside a packet's own output, a padding byte left unwritten or a counter_out that
a seal touched fails as a wrong byte does (tests/wg_support.py).  All comparisons are byte
equality.  The kernel runs with 8 lanes a packet where the call's max_len is at most 2 KiB
and with 16 otherwise; the cases that matter to both say so."""
from __future__ import annotations

import numpy as np
import pytest

import mac_forge as mf
import quic_model as QM
import rfc8439_ref as R
import rfc_batch_support as RB
import wg_ref as W
from gpu_support import dev_bytes, dev_u32, dev_u64, filled, host_bytes, host_np
from quic_support import forge_lanes
from wg_support import COUNTER_EDGES, KEYS3, M, RECEIVERS3, Pkt, WgCase, inner_packet, open_whole, rnd, seal_whole

pytestmark = pytest.mark.gpu

# 8 lanes: Q goes from 1 to 2 at 512 bytes; 16 lanes: at 1,024
LENGTHS_8 = (0, 1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 448, 449, 511, 512, 513, 1420)
LENGTHS_16 = (959, 960, 1023, 1024, 1025, 9000, 16352)
PAD_CAPS = (0, 1420)


def parity_packets(lengths, fill_to=0):
    """Every length four times, the counters and sessions taken in turn (session 5 lies beyond
    the 3-row table: clamped); then drawn lengths up to 1,420 bytes until there are fill_to."""
    pkts = []
    for idx, n in enumerate(lengths):
        for j in range(4):
            i = len(pkts)
            pkts.append(Pkt(inner_packet(n, i), COUNTER_EDGES[(idx + j) % 4], kidx=(0, 1, 2, 5)[(i // 2) % 4]))
    draw = np.random.default_rng(51820).integers(0, 1421, size=max(0, fill_to - len(pkts)))
    for k, n in enumerate(draw.tolist()):
        i = len(pkts)
        pkts.append(Pkt(inner_packet(n, i), 7 * i + (k << 33), kidx=k % 3))
    return pkts


_cases: dict = {}


def parity_case(which: str, pad_cap: int, inplace: bool = False) -> WgCase:
    """"small": the 8-lane lengths and drawn ones, 272 packets (nine workgroups, the last
    ragged); "big": the 16-lane lengths (16 lanes a packet)."""
    key = (which, pad_cap, inplace)
    if key not in _cases:
        pkts = parity_packets(LENGTHS_8, fill_to=272) if which == "small" else parity_packets(LENGTHS_16)
        _cases[key] = WgCase(pkts, pad_cap=pad_cap, inplace=inplace)
    return _cases[key]


@pytest.mark.parametrize("pad_cap", PAD_CAPS)
@pytest.mark.parametrize("which", ("small", "big"))
def test_parity_per_packet_arrays(gpu, which, pad_cap):
    """Seal and open of every length, skew pair, counter edge and session in one batch, whole
    buffers; the open gives every inner packet's length (status 7 for the ones below 20 bytes)."""
    case = parity_case(which, pad_cap)
    assert QM.lanes_for(int(case.lens.max())) == QM.lanes_for(int(case.msg_lens.max())) == (16 if which == "big" else 8)
    if which == "small":
        skews = {(int(a) % 16, int(b) % 16) for a, b in zip(case.raw_off, case.msg_off)}
        assert len(skews) == 256  # input and output skews 0..15, independently
        assert {int(p) for p in case.padded if p % 16} == ({1420} if pad_cap else set())
    assert any(p.kidx >= case.num_keys for p in case.pkts)
    seal_whole(case, where=(which, pad_cap))
    o = open_whole(case, where=(which, pad_cap))
    st = o.arrays["status"].got[:case.count].tolist()
    assert st == [0 if n == 0 or n >= 20 else 7 for n in case.lens.tolist()]
    assert o.arrays["inner_len"].got[:case.count].tolist() == [n if n >= 20 else 0 for n in case.lens.tolist()]


@pytest.mark.parametrize("n,count", ((1215, 1), (60, 31), (61, 32), (1420, 33), (333, 257)))
def test_parity_uniform_fields(gpu, n, count):
    """No per-packet array at all: uniform_len, strides, session 0; a partial last workgroup."""
    pkts = [Pkt(inner_packet(n, i), 2**32 - 3 + i) for i in range(count)]
    p = W.padded_len(n)
    case = WgCase(pkts, strides=(p + 5, 3, p + 32 + 3, 1))  # odd strides from odd bases
    seal_whole(case, uniform=True, where=("uniform", n))
    open_whole(case, uniform=True, where=("uniform", n))


@pytest.mark.parametrize("max_len", (2048, 4096))
def test_ragged_messages(gpu, max_len):
    """Messages whose payload is no multiple of 16 (a peer may send them; a pad_cap that is no
    multiple of 16 makes the seal write them): n = 1, 17, 63, 65 and around a chunk."""
    pkts = [Pkt(inner_packet(n, i), 900 + i, kidx=i % 3) for i, n in enumerate((1, 17, 63, 65, 20, 41, 127, 129, 1419))]
    case = WgCase(pkts, pad_cap=1)  # max(len, 1): no padding at all
    assert case.padded.tolist() == case.lens.tolist()
    seal_whole(case, max_len=max_len - 32, where=("ragged", max_len))
    open_whole(case, max_len=max_len, where=("ragged", max_len))


@pytest.mark.parametrize("pad_cap", PAD_CAPS)
@pytest.mark.parametrize("which", ("small", "big"))
def test_in_place(gpu, which, pad_cap):
    """Seal with out + 16 == in and open with out == in + 16: the payload stays at its address,
    and the whole buffer is the reference's image."""
    case = parity_case(which, pad_cap, inplace=True)
    assert all(int(r) == int(m) + 16 for r, m in zip(case.raw_off, case.msg_off))
    seal_whole(case, where=("in place", which, pad_cap))
    open_whole(case, where=("in place", which, pad_cap))


def flip(msg: bytes, at: int, mask: int = 0x01) -> bytes:
    b = bytearray(msg)
    b[at] ^= mask
    return bytes(b)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n", (0, 16, 1424))
def test_failures(gpu, keep, n):
    """A flipped bit in the header's counter, in the first, middle and last ciphertext byte and
    in the tag: SG_E_BAD_MAC, the output all zero, counter_out 0 and inner_len 0 -- or with
    SG_WG_KEEP_FAILED what the reference decrypts and the wire counter -- and the good packets
    between them untouched.  A flipped receiver index changes nothing: it is not authenticated."""
    flips = [(8, 0x01), (15, 0x80), (16 + n, 0x01), (16 + n + 15, 0x80)]
    if n:
        flips += [(16, 0x01), (16 + n // 2, 0x10), (16 + n - 1, 0x40)]
    pkts = [Pkt(inner_packet(n, i), 77000 + i, kidx=i % 3) for i in range(2 * len(flips) + 2)]
    case = WgCase(pkts)
    msgs = [case.protected(i) for i in range(case.count)]
    want_bad = []
    for k, (at, mask) in enumerate(flips):
        msgs[2 * k + 1] = flip(msgs[2 * k + 1], at, mask)
        want_bad.append(2 * k + 1)
    msgs[-1] = flip(msgs[-1], 5, 0xFF)
    for inplace in (False, True):
        c = case if not inplace else WgCase(pkts, inplace=True)
        o = open_whole(c, msgs, keep=keep, where=("failures", n, keep, inplace))
        st = o.arrays["status"].got[:case.count].tolist()
        good = 7 if n == 16 else 0  # 16 bytes hold no IP header: authentic, SG_STATUS_BAD_INNER
        assert st == [1 if i in want_bad else good for i in range(case.count)]


def test_header_short_and_skipped(gpu):
    """Type bytes 01 00 00 00 and 04 00 00 01 are SG_STATUS_BAD_HEADER and nothing is written;
    len 0 and 31 are SG_E_SHORT, 32 is a keepalive; a packet of max_len + 1 bytes is
    SG_STATUS_SKIPPED in both directions, nothing of it touched, and the call returns SG_OK.
    The order: skipped before short before the header."""
    lens_in = (100, 100, 100, 0, 0, 0, 305, 300, 40)
    pkts = [Pkt(inner_packet(n, i), 5 + i, kidx=i % 3) for i, n in enumerate(lens_in)]
    case = WgCase(pkts)
    seal_whole(case, max_len=300, exp_st=[0, 0, 0, 0, 0, 0, 3, 0, 0], where=("skipped",))
    msgs = [case.protected(i) for i in range(case.count)]
    msgs[1] = b"\x01\0\0\0" + msgs[1][4:]
    msgs[2] = b"\x04\0\0\x01" + msgs[2][4:]
    lens = [len(m) for m in msgs]
    lens[3], lens[4] = 0, 31
    msgs[8] = b"\x01" + msgs[8][1:]  # a wrong type in a message that is cut short: short
    lens[8] = 20
    max_len = 32 + 304
    for inplace in (False, True):
        c = case if not inplace else WgCase(pkts, inplace=True)
        o = open_whole(c, msgs, lens=lens, max_len=max_len, where=("header", inplace))
        assert o.arrays["status"].got[:case.count].tolist() == [0, 6, 6, 2, 2, 0, 3, 0, 2]
        assert o.arrays["inner_len"].got[5] == 0 and o.arrays["counter_out"].got[5] == 10
    # a wrong type in a message longer than max_len: skipped
    msgs[7] = b"\x01" + msgs[7][1:]
    o = open_whole(case, msgs, lens=lens, max_len=32 + 112, where=("order",))
    assert o.arrays["status"].got[:case.count].tolist() == [0, 6, 6, 2, 2, 0, 3, 3, 2]


def test_inner_length(gpu):
    """IPv4 and IPv6 headers with L at both edges, 0 and 15 bytes of padding behind L, version
    5, too little room for a header: SG_STATUS_BAD_INNER leaves plaintext and counter in place;
    with inner_len == NULL nothing is parsed and every good tag is SG_OK."""
    # the edges of L, on messages without padding (pad_cap 1): the plaintext is the inner packet
    inners, want = [], []
    for n in (20, 32, 33, 48, 1424):
        for L, ok in ((19, False), (20, True), (n, True), (n + 1, False)):
            inners.append(W.ipv4(L, n)); want.append(L if ok else None)
    for n in (40, 48, 49, 64, 1440):
        for pl, ok in ((0, True), (n - 40, True), (n - 39, False)):
            inners.append(W.ipv6(pl, n)); want.append(40 + pl if ok else None)
    inners += [bytes([0x55]) + W.ipv4(20, 63)[1:], W.ipv6(0, 39), W.ipv4(16, 16), W.ipv4(19, 19), b"", bytes(64)]
    want += [None, None, None, None, 0, None]
    edges = [Pkt(x, 2**40 + i, kidx=i % 3) for i, x in enumerate(inners)]
    # 0, 7, 11 and 15 bytes of padding behind L
    inners = [W.ipv4(32, 32), W.ipv4(21, 21), W.ipv4(33, 33), W.ipv6(8, 48), W.ipv6(1, 41), W.ipv6(9, 49), W.ipv4(17, 17)]
    padded = [Pkt(x, 2**50 + i, kidx=i % 3) for i, x in enumerate(inners)]
    for pkts, pad_cap, want in ((edges, 1, want), (padded, 0, [32, 21, 33, 48, 41, 49, None])):
        for inplace in (False, True):
            case = WgCase(pkts, pad_cap=pad_cap, inplace=inplace)
            assert pad_cap == 0 or case.padded.tolist() == case.lens.tolist()
            o = open_whole(case, where=("inner", pad_cap, inplace))
            assert o.arrays["status"].got[:case.count].tolist() == [7 if w is None else 0 for w in want]
            assert o.arrays["inner_len"].got[:case.count].tolist() == [w or 0 for w in want]
            assert o.arrays["counter_out"].got[:case.count].tolist() == [p.counter for p in pkts]
            o = open_whole(case, want_inner=False, where=("inner NULL", pad_cap, inplace))
            assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count


def forged_message(key, counter, ct):
    """The message of a chosen ciphertext: its tag by the sequential reference."""
    return W.header_of(RECEIVERS3[0], counter) + ct + R.tag_of(key, W.nonce_of(counter), b"", ct)


@pytest.mark.parametrize("max_len", (2048, 4096))
def test_mac_finish_edges(gpu, max_len):
    """Messages whose ciphertext drives the Poly1305 accumulator to mac_forge.TARGETS (p - 1 ..
    p - 5, 2^128 -+, 2^129, the all-zero and all-ones tags), at a 1,200-byte and a 64-byte
    payload, opened by the 8-lane (max_len 2048) and the 16-lane kernel: status 0 and the
    reference's plaintext; and sealed to the same bytes."""
    key = KEYS3[:32]
    pkts, msgs = [], []
    for n in (1200, 64):
        for name, T in mf.TARGETS.items():
            counter = 4000 + len(pkts)
            nonce = W.nonce_of(counter)
            r, s = RB.poly_rs(key, nonce)
            target = (T(r, s, None) if callable(T) else T) % RB.P
            ct, _ = RB.forge_ct(key, nonce, b"", n, target, f"wg {name} {n}")
            assert RB.accumulator(key, nonce, b"", ct) == target
            if name in mf.TAG_PATTERN:
                assert R.tag_of(key, nonce, b"", ct) == mf.TAG_PATTERN[name]
            pkts.append(Pkt(R.xor_stream(key, nonce, ct), counter))
            msgs.append(forged_message(key, counter, ct))
    case = WgCase(pkts)
    assert [case.protected(i) for i in range(case.count)] == msgs  # the forged ciphertext is what sealing its plaintext gives
    o = open_whole(case, msgs, max_len=max_len, want_inner=False, where=("finish", max_len))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    seal_whole(case, max_len=max_len - 32, where=("finish", max_len))


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("tname", ("m1", "zero"))
def test_mac_lane_sums(gpu, max_len, tname):
    """Every per-lane sum of the kernel's MAC, and the tail slot's, forged to p - 1 (all limbs
    at their maximum) and to 0.  With an empty AD no lane is left unsteered: skipped is 0."""
    G = QM.lanes_for(max_len)
    key = KEYS3[32:64]
    pkts, msgs = [], []
    for k, n in enumerate((1248, 96, 64 * (G + 3) + 48)):
        counter = 9000 + k
        nonce = W.nonce_of(counter)
        ct, tries, skipped = forge_lanes(key, nonce, b"", n, G, mf.B_TARGETS[tname], f"wg {tname} {n} {G}")
        assert skipped == 0
        r, _ = RB.poly_rs(key, nonce)
        H, ts = QM.lane_sums(R.mac_stream(b"", ct), 0, n, r, G)
        sets = QM.lane_sets(0, n, G)[:-1]
        assert ts == mf.B_TARGETS[tname] and all(H[t] == mf.B_TARGETS[tname] for t, _ in sets)
        assert len(sets) == -(-(n // 64) // QM.geom(n, G)[1])
        assert QM.tag(key, nonce, b"", ct, G) == R.tag_of(key, nonce, b"", ct)
        pkts.append(Pkt(R.xor_stream(key, nonce, ct), counter, kidx=1))
        msgs.append(W.header_of(RECEIVERS3[1], counter) + ct + R.tag_of(key, nonce, b"", ct))
    case = WgCase(pkts)
    assert [case.protected(i) for i in range(3)] == msgs
    o = open_whole(case, msgs, max_len=max_len, want_inner=False, where=("lanes", max_len, tname))
    assert o.arrays["status"].got[:3].tolist() == [0, 0, 0]
    seal_whole(case, max_len=max_len - 32, where=("lanes", max_len, tname))


def test_graph_capture(gpu):
    """One seal and one open captured on a single stream and replayed once: the bytes of the
    direct calls."""
    import torch

    from suruga_amd import wg as WG

    count = 300
    pkts = [Pkt(inner_packet(1200 - i % 7, i), 50000 + 3 * i, kidx=i % 3) for i in range(count)]
    case = WgCase(pkts, pad_cap=1420)
    inp = torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda")
    for o, p in zip(case.raw_off, pkts):
        inp[int(o):int(o) + len(p.inner)] = dev_bytes(p.inner)
    tables = dict(keys=dev_bytes(KEYS3), key_index=dev_u32([p.kidx for p in pkts]))
    receiver, counter = dev_u32(RECEIVERS3), dev_u64([p.counter for p in pkts])
    lens, mlens = dev_u32(case.lens), dev_u32(case.msg_lens)
    raw_off, msg_off = dev_u64(case.raw_off), dev_u64(case.msg_off)

    def run(ct, back, st, ctr_out, ilen, stream):
        WG.seal_wg(WG.WgBatch(count=count, inp=inp, out=ct, status=st[:count], lens=lens, max_len=1300, in_off=raw_off,
                              out_off=msg_off, receiver=receiver, counter=counter, pad_cap=1420, stream=stream, **tables))
        WG.open_wg(WG.WgBatch(count=count, inp=ct, out=back, status=st[count:], counter_out=ctr_out, inner_len=ilen,
                              lens=mlens, max_len=1300, in_off=msg_off, out_off=raw_off, stream=stream, **tables))

    def buffers():
        return (torch.zeros(case.msg_size + 16, dtype=torch.uint8, device="cuda"),
                torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda"), filled(2 * count, 0xFF),
                torch.full((count,), -1, dtype=torch.int64, device="cuda"),
                torch.full((count,), -1, dtype=torch.int32, device="cuda"))

    direct, captured = buffers(), buffers()
    run(*direct, None)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(*captured, torch.cuda.current_stream())
    for t in captured[:2]:
        t.zero_()
    captured[2].fill_(0xFF)
    captured[3].fill_(-1)
    captured[4].fill_(-1)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(direct, captured):
        assert bool(torch.equal(a, b))
    ct_h, back_h = host_bytes(direct[0]), host_bytes(direct[1])
    assert host_bytes(direct[2]) == bytes(2 * count)
    assert host_np(direct[3]).tolist() == [p.counter for p in pkts]
    assert host_np(direct[4]).tolist() == case.lens.tolist()
    for i in range(0, count, 13):
        lo = int(case.msg_off[i])
        assert ct_h[lo:lo + len(case.protected(i))] == case.protected(i)
        lo = int(case.raw_off[i])
        assert back_h[lo:lo + len(pkts[i].inner)] == pkts[i].inner


def test_round_trip_zipf(gpu):
    """wg.py end to end: 4,096 packets of Zipf lengths through seal, then open in place; the
    counters, the inner lengths and the packets come back, and a few messages are the
    reference's."""
    import torch

    import suruga_amd as S
    from suruga_amd import workloads as WL

    count, sessions, cap = 4096, 7, 1420
    k = WL.zipf_lengths(count) // 64
    lens = np.clip(64 * k - 63 + (13 * np.arange(count)) % 64, 20, 16352).astype(np.uint32)
    mlens = np.array([W.message_len(int(n), cap) for n in lens], dtype=np.uint32)
    assert int(lens.max()) > 2048 and all(S.message_len(int(n), cap) == int(m) for n, m in zip(lens[:64], mlens[:64]))
    slot = (mlens.astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(16)
    msg_off = np.concatenate(([0], np.cumsum(slot)[:-1])).astype(np.uint64) + (np.arange(count, dtype=np.uint64) % np.uint64(16))
    size = int(msg_off[-1] + slot[-1]) + 16
    host = np.random.default_rng(4096).integers(0, 256, size=size, dtype=np.uint8)
    for i in range(count):  # an IPv4 header's first four bytes in front of every inner packet
        o = int(msg_off[i]) + 16
        host[o], host[o + 2], host[o + 3] = 0x45, int(lens[i]) >> 8, int(lens[i]) & 0xFF
    keys = b"".join(R.data(32, b"wg session %d" % j) for j in range(sessions))
    receivers = [0x1000 + j for j in range(sessions)]
    kidx = np.arange(count) % sessions
    counters = [2**32 - 2000 + 3 * i for i in range(count)]
    buf = torch.from_numpy(host.copy()).to("cuda")
    st, ctr_out, ilen = filled(count, 0xFF), dev_u64([0] * count), dev_u32([0] * count)
    common = dict(count=count, keys=dev_bytes(keys), key_index=dev_u32(kidx), status=st)
    S.seal_wg(S.WgBatch(inp=buf[16:], out=buf, receiver=dev_u32(receivers), counter=dev_u64(counters), pad_cap=cap,
                        lens=dev_u32(lens), max_len=16352, in_off=dev_u64(msg_off), out_off=dev_u64(msg_off), **common))
    torch.cuda.synchronize()
    assert host_bytes(st) == bytes(count)
    sealed = host_np(buf)
    for i in (0, 1, 777, int(np.argmax(lens)), count - 1):
        o, n = int(msg_off[i]), int(lens[i])
        want = W.protect(keys[32 * int(kidx[i]):32 * int(kidx[i]) + 32], receivers[int(kidx[i])], counters[i],
                         host[o + 16:o + 16 + n].tobytes(), cap)
        assert sealed[o:o + int(mlens[i])].tobytes() == want, i
    st.fill_(0xFF)
    S.open_wg(S.WgBatch(inp=buf, out=buf[16:], counter_out=ctr_out, inner_len=ilen, lens=dev_u32(mlens), max_len=16384,
                        in_off=dev_u64(msg_off), out_off=dev_u64(msg_off), **common))
    torch.cuda.synchronize()
    assert host_bytes(st) == bytes(count)
    assert host_np(ctr_out).tolist() == counters and host_np(ilen).tolist() == lens.tolist()
    back = host_np(buf)
    for i in range(count):
        o, n = int(msg_off[i]) + 16, int(lens[i])
        assert np.array_equal(back[o:o + n], host[o:o + n]), i
        assert not back[o + n:o + int(mlens[i]) - 32].any(), i  # the padding came back as zeros
