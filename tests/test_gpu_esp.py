"""sg_seal_batch_esp / sg_open_batch_esp (sg_esp.hip) on the GPU against tests/esp_ref.py.

Every data buffer sits in a footprint.sentinel buffer with a margin in front and behind and
is compared whole afterwards, with the status bytes, seq_out, payload_len and
next_header_out, so a byte written outside a packet's own output, a padding byte left
unwritten or a seq_out that a seal touched fails as a wrong byte does
(tests/esp_support.py).  All comparisons are byte equality.  The kernel runs with 8 lanes a
packet where the call's max_len is at most 2 KiB and with 16 otherwise; the cases that
matter to both say so."""
from __future__ import annotations

import numpy as np
import pytest

import esp_ref as E
import mac_forge as mf
import quic_model as QM
import quic_support as QS
import rfc8439_ref as R
import rfc_batch_support as RB
from esp_support import KEYS4, NEXT_HEADERS, SALTS4, SEQ_EDGES, SPIS4, EspCase, Pkt, open_whole, rnd, seal_whole
from gpu_support import dev_bytes, dev_u8, dev_u32, dev_u64, filled, host_bytes, host_np

pytestmark = pytest.mark.gpu

# With align 4 and P = len + pad + 2: len 58..66 put the trailer wholly into the tail (P 60),
# into the last whole chunk with no tail behind it (62 -> P 64) and into a tail that holds
# nothing else (63 -> P 68; P is a multiple of 4, so the two trailer bytes are never split),
# and 8 lanes step Q at P = 512 (len 446..450 around 448, 510..514 around 512).
LENGTHS_8 = (0, 1, 2, 3, *range(58, 67), *range(446, 451), *range(510, 515), 1438)
LENGTHS_16 = (*range(958, 963), *range(1022, 1027), 9000, 16350)
ALIGNS = (4, 16)


def parity_packets(lengths, fill_to=0):
    """Every length four times, the SAs taken in turn (SA 7 lies beyond the 4-row table:
    clamped to row 3), each SA at its sequence number edge, every other packet with an IV of
    its own; then drawn lengths up to 1,438 bytes until there are fill_to."""
    pkts = []

    def add(n, kidx):
        i = len(pkts)
        iv = None if i % 2 == 0 else (0xA5A5A5A500000000 ^ (i * 0x0101010101010101)) & (2**64 - 1)
        pkts.append(Pkt(rnd(n, f"esp payload {n} {i}"), SEQ_EDGES[min(kidx, 3)], kidx=kidx, nh=NEXT_HEADERS[i % 6], iv=iv))

    for n in lengths:
        for j in range(4):
            add(n, (0, 1, 2, 7, 3)[(len(pkts) // 2 + j) % 5])
    for k, n in enumerate(np.random.default_rng(4303).integers(0, 1439, size=max(0, fill_to - len(pkts))).tolist()):
        add(n, k % 4)
    return pkts


_cases: dict = {}


def parity_case(which: str, align: int, esn: bool, inplace: bool = False) -> EspCase:
    """"small": the 8-lane lengths and drawn ones, 272 packets (nine workgroups, the last
    partial); "big": the 16-lane lengths (16 lanes a packet)."""
    key = (which, align, esn, inplace)
    if key not in _cases:
        pkts = parity_packets(LENGTHS_8, fill_to=272) if which == "small" else parity_packets(LENGTHS_16)
        _cases[key] = EspCase(pkts, align=align, esn=esn, inplace=inplace)
    return _cases[key]


@pytest.mark.parametrize("esn", (False, True))
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("which", ("small", "big"))
def test_parity_per_packet_arrays(gpu, which, align, esn):
    """Seal and open of every length, skew pair, sequence number edge and SA in one batch, whole
    buffers; the open gives every payload's length and next header and the 64-bit numbers."""
    case = parity_case(which, align, esn)
    assert QM.lanes_for(int(case.lens.max())) == QM.lanes_for(int(case.pkt_lens.max())) == (16 if which == "big" else 8)
    if which == "small":
        skews = {(int(a) % 16, int(b) % 16) for a, b in zip(case.raw_off, case.msg_off)}
        assert len(skews) == 256 and case.count % 32 != 0  # input and output skews 0..15 independently; a partial last workgroup
        if align == 4:
            assert {0, 4, 60} <= {int(p) % 64 for p in case.padded} and {0, 1, 2, 3} == {int(p - n - 2) for p, n in zip(case.padded, case.lens)}
    assert any(p.kidx >= case.num_sas for p in case.pkts) and {case.row(i) for i in range(case.count)} == {0, 1, 2, 3}
    seal_whole(case, where=(which, align, esn))
    o = open_whole(case, where=(which, align, esn))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    assert o.arrays["payload_len"].got[:case.count].tolist() == case.lens.tolist()
    assert o.arrays["next_header_out"].got[:case.count].tolist() == [p.nh for p in case.pkts]
    assert o.arrays["seq_out"].got[:case.count].tolist() == [case.seq(i) for i in range(case.count)]


def wide_lengths(align):
    """Payload lengths whose padding is 0, 1, 62, 63, 254, 255 (as far as the align has them)
    and the align's largest, at one to six aligns of P: the padding crosses one and several
    chunk and lane boundaries, whole chunks are made, and len 0 comes with the largest padding."""
    lens = {0}
    for pad in (0, 1, 2, 62, 63, 65, 130, 254, 255, align - 2, align - 1):
        if pad < align:
            lens |= {align * m - 2 - pad for m in (1, 2, 3, 6) if align * m - 2 - pad >= 0}
    return sorted(lens)


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("align,esn", ((64, False), (256, True), (252, False), (68, True)))
def test_wide_padding(gpu, align, esn, max_len):
    """Up to 255 bytes of padding made in the kernel: cuts anywhere in a chunk, whole chunks
    without a byte of input, with (align 68, 252) and without (64, 256) a tail; 8 and 16 lanes.
    The input holds sentinel bytes directly behind every payload, which the output must not
    depend on: it is the reference's, which never saw them."""
    lens = wide_lengths(align)
    pkts = [Pkt(rnd(n, f"esp wide {align} {n}"), SEQ_EDGES[i % 4] - (i % 3 if i % 4 else 0), kidx=i % 4, nh=NEXT_HEADERS[i % 6],
                iv=None if i % 3 else 7 * i + (i << 40)) for i, n in enumerate(lens)]
    case = EspCase(pkts, align=align, esn=esn)
    pads = {int(p - n - 2) for p, n in zip(case.padded, case.lens)}
    assert pads >= {0, 1, 62, 63, align - 2, align - 1} and max(pads) == align - 1
    if align == 256:
        assert pads >= {254, 255} and int(case.padded[0]) == 256 and case.lens[0] == 0  # a payload of 0 bytes with pad 254
    assert any(int(p) % 64 for p in case.padded) == (align % 64 != 0)  # a tail, or none in the whole batch
    if align >= 252:  # whole chunks made: two and more without a byte of input
        assert any(int(p) // 64 - -(-int(n) // 64) >= 2 for p, n in zip(case.padded, case.lens))
    for inplace in (False, True):
        c = case if not inplace else EspCase(pkts, align=align, esn=esn, inplace=True)
        seal_whole(c, max_len=max_len - 34, where=("wide", align, max_len, inplace))
        o = open_whole(c, max_len=max_len, where=("wide", align, max_len, inplace))
        assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
        assert o.arrays["payload_len"].got[:case.count].tolist() == case.lens.tolist()


@pytest.mark.parametrize("n,count,align,esn", ((1215, 1, 4, False), (60, 31, 4, True), (61, 32, 16, False), (1438, 33, 4, True),
                                               (333, 257, 64, True)))
def test_parity_uniform_fields(gpu, n, count, align, esn):
    """No per-packet array but seq: uniform_len, uniform_next_header, strides, SA 0, the IV the
    sequence number; a partial last workgroup."""
    top = 2**32 + 60  # the window of 64 starts at the first packet's number
    pkts = [Pkt(rnd(n, f"esp uniform {n} {i}"), 2**32 - 3 + i, nh=59) for i in range(count)]
    p = E.padded_len(n, align)
    case = EspCase(pkts, align=align, esn=esn, tops=(top,) * 4, strides=(p + 5, 3, p + 32 + 3, 1))  # odd strides from odd bases
    seal_whole(case, uniform=True, where=("uniform", n))
    o = open_whole(case, uniform=True, where=("uniform", n))
    assert o.arrays["status"].got[:count].tolist() == [0] * count
    assert o.arrays["seq_out"].got[:count].tolist() == [case.seq(i) for i in range(count)]


@pytest.mark.parametrize("esn", (False, True))
@pytest.mark.parametrize("align", ALIGNS)
@pytest.mark.parametrize("which", ("small", "big"))
def test_in_place(gpu, which, align, esn):
    """Seal with out + 16 == in and open with out == in + 16: the payload stays at its address,
    and the whole buffer is the reference's image."""
    case = parity_case(which, align, esn, inplace=True)
    assert all(int(r) == int(m) + 16 for r, m in zip(case.raw_off, case.msg_off))
    seal_whole(case, where=("in place", which, align, esn))
    o = open_whole(case, where=("in place", which, align, esn))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count


def flip(msg: bytes, at: int, mask: int = 0x01) -> bytes:
    b = bytearray(msg)
    b[at] ^= mask
    return bytes(b)


@pytest.mark.parametrize("keep", (False, True))
@pytest.mark.parametrize("n,esn", ((0, False), (14, True), (1438, True)))
def test_failures(gpu, keep, n, esn):
    """A flipped bit in the sequence number, the IV, the first, middle and last ciphertext byte
    and the ICV, and under ESN an SA whose replay_top infers a high half one off although no
    wire bit changed: SG_E_BAD_MAC, the output all zero, seq_out, payload_len and
    next_header_out 0 -- or with SG_ESP_KEEP_FAILED what the reference decrypts and the inferred
    sequence number -- and the good packets between them untouched."""
    P = E.padded_len(n)
    flips = [(4, 0x80), (7, 0x01), (8, 0x01), (15, 0x80), (16, 0x01), (16 + P // 2, 0x10), (16 + P - 1, 0x40), (16 + P, 0x01),
             (16 + P + 15, 0x80)]
    count = 2 * len(flips) + 4
    # SAs 0..2 sit at 5 * 2^32 + 1000; SA 3's receiver believes itself one subspace on
    tops = (5 * 2**32 + 1000,) * 3 + (6 * 2**32 + 1000,)
    pkts = [Pkt(rnd(n, f"esp fail {n} {i}"), 5 * 2**32 + 990 + i % 8, kidx=i % 3, nh=NEXT_HEADERS[i % 6]) for i in range(count)]
    pkts[-2].kidx = pkts[-4].kidx = 3
    case = EspCase(pkts, esn=esn, tops=tops)
    msgs = [case.protected(i) for i in range(case.count)]
    want_bad = []
    for k, (at, mask) in enumerate(flips):
        msgs[2 * k + 1] = flip(msgs[2 * k + 1], at, mask)
        want_bad.append(2 * k + 1)
    if esn:
        want_bad += [count - 4, count - 2]
    for inplace in (False, True):
        c = case if not inplace else EspCase(pkts, esn=esn, tops=tops, inplace=True)
        o = open_whole(c, msgs, keep=keep, where=("failures", n, keep, inplace))
        assert o.arrays["status"].got[:case.count].tolist() == [1 if i in want_bad else 0 for i in range(case.count)]
        if esn and keep:
            assert int(o.arrays["seq_out"].got[count - 2]) == pkts[-2].seq + 2**32


def test_header_short_and_skipped(gpu):
    """A wrong SPI (another SA's, one bit off) is SG_STATUS_BAD_HEADER and nothing is written;
    len 0 and 33 are SG_E_SHORT, 34 holds a trailer alone; a packet of max_len + 1 bytes is
    SG_STATUS_SKIPPED in both directions, nothing of it touched, and the call returns SG_OK.
    The order: skipped before short before the header."""
    lens_in = (100, 100, 100, 0, 0, 2, 305, 298, 40)
    pkts = [Pkt(rnd(n, f"esp hdr {i}"), 5 + i, kidx=i % 3, nh=6) for i, n in enumerate(lens_in)]
    pkts[5] = Pkt(b"", 10, kidx=2, plain=b"\x00\x3b")  # 34 bytes: no padding, next header 59, an empty payload
    sealable = EspCase(pkts[:5] + [Pkt(b"", 10, kidx=2)] + pkts[6:])
    seal_whole(sealable, max_len=300, exp_st=[0, 0, 0, 0, 0, 0, 3, 0, 0], where=("skipped",))
    case = EspCase(pkts)
    msgs = [case.protected(i) for i in range(case.count)]
    assert len(msgs[5]) == 34 and len(msgs[7]) == 332
    msgs[1] = E.header_of(SPIS4[2], 6, 6)[:4] + msgs[1][4:]
    msgs[2] = flip(msgs[2], 3, 0x01)
    lens = [len(m) for m in msgs]
    lens[3], lens[4] = 0, 33
    msgs[8] = flip(msgs[8], 0, 0x80)  # a wrong SPI in a packet that is cut short: short
    lens[8] = 20
    max_len = 32 + 304
    for inplace in (False, True):
        c = case if not inplace else EspCase(pkts, inplace=True)
        o = open_whole(c, msgs, lens=lens, max_len=max_len, where=("header", inplace))
        assert o.arrays["status"].got[:case.count].tolist() == [0, 6, 6, 2, 2, 0, 3, 0, 2]
        assert o.arrays["payload_len"].got[5] == 0 and o.arrays["next_header_out"].got[5] == 59 and o.arrays["seq_out"].got[5] == 10
    # a wrong SPI in a packet longer than max_len: skipped
    msgs[7] = flip(msgs[7], 1, 0x04)
    o = open_whole(case, msgs, lens=lens, max_len=32 + 112, where=("order",))
    assert o.arrays["status"].got[:case.count].tolist() == [0, 6, 6, 2, 2, 0, 3, 3, 2]


@pytest.mark.parametrize("max_len", (2048, 4096))
def test_trailer(gpu, max_len):
    """Authentic packets with trailers no seal writes: a pad byte wrong at the first, a middle
    and the last position, over 3 and over 200 bytes of padding (every lane's share), pad + 2 ==
    n (all padding, an empty payload: valid), pad + 2 == n + 1, pad 255 in a 34-byte packet:
    SG_STATUS_BAD_INNER leaves plaintext and seq_out in place; with payload_len == NULL nothing
    is parsed and every good ICV is SG_OK."""
    plains, want = [], []

    def add(body, padding, pad, nh, ok):
        plains.append(bytes(body) + bytes(padding) + bytes([pad, nh]))
        want.append((len(body), nh) if ok else None)

    for nbody, pad in ((40, 3), (7, 200), (300, 255), (64, 62)):
        body, good = rnd(nbody, f"esp trailer {nbody}"), bytes(range(1, pad + 1))
        add(body, good, pad, 17, True)
        for at in (0, pad // 2, pad - 1):
            add(body, good[:at] + bytes([good[at] ^ 0x80]) + good[at + 1:], pad, 17, False)
        add(body, bytes(pad), pad, 17, False)             # zeros, as WireGuard pads
        add(body, bytes(range(pad)), pad, 17, False)      # 0, 1, 2 ..: one off throughout
    add(b"", bytes(range(1, 11)), 10, 59, True)           # pad + 2 == n
    add(b"", bytes(range(2, 11)), 10, 59, False)          # pad + 2 == n + 1
    add(b"", bytes(range(1, 254)), 253, 4, True)
    add(b"", bytes(range(2, 255)), 254, 4, False)         # pad + 2 == n + 2
    add(b"", b"", 255, 4, False)                          # pad 255 in a 34-byte packet
    add(b"", b"", 1, 4, False)
    add(b"", b"", 0, 4, True)
    add(rnd(70, "esp trailer body"), b"", 0, 0, True)
    pkts = [Pkt(b"", 2**40 + i, kidx=i % 4, plain=x, iv=i) for i, x in enumerate(plains)]
    tops = (2**40 + 1000,) * 4
    for esn, inplace in ((False, False), (True, True)):
        case = EspCase(pkts, esn=esn, tops=tops, window=2**31, inplace=inplace)
        o = open_whole(case, max_len=max_len, where=("trailer", esn, inplace))
        assert o.arrays["status"].got[:case.count].tolist() == [7 if w is None else 0 for w in want]
        assert o.arrays["payload_len"].got[:case.count].tolist() == [w[0] if w else 0 for w in want]
        assert o.arrays["next_header_out"].got[:case.count].tolist() == [w[1] if w else 0 for w in want]
        assert o.arrays["seq_out"].got[:case.count].tolist() == [case.seq(i) for i in range(case.count)]
        o = open_whole(case, max_len=max_len, want_trailer=False, where=("trailer NULL", esn, inplace))
        assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count


@pytest.mark.parametrize("window", (1, 64, 2**31))
def test_esn_inference(gpu, window):
    """RFC 4303 appendix A2.1 on the device: per SA a top T in case A (Tl >= W - 1) or case B,
    and packets sealed with the 64-bit numbers at both ends of [T - W + 1, T - W + 1 + 2^32)
    and on both sides of T -- seq_lo = Bl - 1, Bl and Bl + 1 among them: every one opens, and
    seq_out is the sealed number.  The number just below the interval has the low bits of its
    last one: inferred as that, it fails its ICV."""
    tops = ((5 << 32) | (window - 1 + 1000), (5 << 32) | ((window - 2) & E.M32 if window > 1 else 0),
            (1 << 32) | (window - 1), (0xFFFFFFFE << 32) | 0xFFFFFFFF)
    pkts, inside = [], []
    for r, top in enumerate(tops):
        start = top - window + 1
        seqs = [start, start + 1, start + 2**32 - 1, start + 2**32 - 2, top, top + 1, top + 2**31, start - 1]
        if window > 1:
            seqs += [top - 1, start + window // 2]
        for s in seqs:
            pkts.append(Pkt(rnd(30 + len(pkts), f"esp esn {window} {len(pkts)}"), s, kidx=r, nh=41))
            inside.append(start <= s < start + 2**32)
    case = EspCase(pkts, esn=True, tops=tops, window=window)
    assert {(t & E.M32) >= window - 1 for t in tops} == ({True, False} if window > 1 else {True})
    lows = {(case.row(i), (p.seq - (tops[case.row(i)] - window + 1)) & E.M32) for i, p in enumerate(pkts)}
    assert all({(r, 0), (r, 1), (r, E.M32)} <= lows for r in range(4))  # Bl, Bl + 1 and Bl - 1
    seal_whole(case, where=("esn", window))
    for keep in (False, True):
        o = open_whole(case, keep=keep, where=("esn", window, keep))
        assert o.arrays["status"].got[:case.count].tolist() == [0 if ok else 1 for ok in inside]
        got = o.arrays["seq_out"].got[:case.count].tolist()
        assert all(g == p.seq for g, p, ok in zip(got, pkts, inside) if ok)
        if keep:
            assert all(g == p.seq + 2**32 for g, p, ok in zip(got, pkts, inside) if not ok)


def steer(key, nonce, ad, ct, target, fixed: bytes, seed: str):
    """ct (from rfc_batch_support.forge_ct) with its last bytes replaced by `fixed` and its
    first block solved again for the same accumulator; the second block is drawn again until
    the solution is a block value."""
    ct = bytearray(ct)
    ct[len(ct) - len(fixed):] = fixed
    r, _ = RB.poly_rs(key, nonce)
    na = (len(ad) + 15) // 16
    for t in range(200):
        ct[:16] = bytes(16)
        stream = R.mac_stream(ad, bytes(ct))
        B = len(stream) // 16
        c = (target - RB.accumulator(key, nonce, ad, bytes(ct))) * pow(pow(r, B - na, RB.P), -1, RB.P) % RB.P
        if c < (1 << 128):
            ct[:16] = c.to_bytes(16, "little")
            return bytes(ct)
        ct[16:32] = rnd(16, f"steer {seed} {t}")
    raise AssertionError("no forgery in 200 tries")


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("esn", (False, True))
def test_mac_finish_edges(gpu, max_len, esn):
    """Packets whose ciphertext drives the Poly1305 accumulator to mac_forge.TARGETS (p - 1 ..
    p - 5, 2^128 -+, 2^129, the all-zero and all-ones tags) behind the 8- and the 12-byte AD, at
    a 1,200-byte and a 64-byte ciphertext, opened by the 8-lane (max_len 2048) and the 16-lane
    kernel: status 0 and the reference's plaintext.  The same with the last two plaintext
    bytes made a trailer (no padding, some next header) and the first block solved again:
    sealed to the same bytes, and opened with the trailer parsed."""
    key, salt, spi = KEYS4[:32], SALTS4[:4], SPIS4[0]
    plain, sealable, msgs = [], [], []
    for n in (1200, 64):
        for name, T in mf.TARGETS.items():
            seq = 2**33 + 4000 + len(plain)
            nonce, ad = E.nonce_of(salt, seq), E.ad_of(spi, seq if esn else seq & E.M32, esn)
            r, s = RB.poly_rs(key, nonce)
            target = (T(r, s, None) if callable(T) else T) % RB.P
            ct, _ = RB.forge_ct(key, nonce, ad, n, target, f"esp {name} {n} {esn}")
            assert RB.accumulator(key, nonce, ad, ct) == target
            if name in mf.TAG_PATTERN:
                assert R.tag_of(key, nonce, ad, ct) == mf.TAG_PATTERN[name]
            assert QM.tag(key, nonce, ad, ct, QM.lanes_for(max_len)) == R.tag_of(key, nonce, ad, ct)
            plain.append(Pkt(b"", seq, plain=R.xor_stream(key, nonce, ct), iv=seq))
            msgs.append(E.header_of(spi, seq, seq) + ct + R.tag_of(key, nonce, ad, ct))
            # ... and with a trailer: the ciphertext of 00 || next header under the last two bytes
            nh = len(plain) & 0xFF
            ks = R.xor_stream(key, nonce, bytes(n))
            ct2 = steer(key, nonce, ad, ct, target, bytes([ks[n - 2], ks[n - 1] ^ nh]), f"{name} {n} {esn}")
            assert RB.accumulator(key, nonce, ad, ct2) == target
            pt2 = R.xor_stream(key, nonce, ct2)
            assert pt2[-2:] == bytes([0, nh])
            sealable.append(Pkt(pt2[:-2], seq, nh=nh, iv=seq))
    tops = (2**33 + 4010,) * 4
    case = EspCase(plain, esn=esn, tops=tops)
    assert [case.protected(i) for i in range(case.count)] == msgs
    o = open_whole(case, msgs, max_len=max_len, want_trailer=False, where=("finish", max_len, esn))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    case = EspCase(sealable, esn=esn, tops=tops)
    seal_whole(case, max_len=max_len - 34, where=("finish", max_len, esn))
    o = open_whole(case, max_len=max_len, where=("finish trailer", max_len, esn))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count


@pytest.mark.parametrize("max_len", (2048, 4096))
@pytest.mark.parametrize("esn", (False, True))
@pytest.mark.parametrize("tname", ("m1", "zero"))
def test_mac_lane_sums(gpu, max_len, esn, tname):
    """Every per-lane sum of the kernel's MAC, and the tail slot's, forged to p - 1 (all limbs
    at their maximum) and to 0.  A lane that holds the additional data alone cannot be steered:
    forge_lanes reports it, and the model says where that is so.  n % 16 == 4: the last four
    ciphertext bytes lie in no whole block and stay as drawn, so a seed whose draw decrypts to
    pad length 0 gives a packet that a seal writes."""
    G = QM.lanes_for(max_len)
    key, salt, spi = KEYS4[32:64], SALTS4[4:8], SPIS4[1]
    pkts, msgs = [], []
    for k, n in enumerate((1252, 100, 64 * (G + 3) + 52, 64 * G + 36)):
        seq = 2**34 + 9000 + k
        nonce, ad = E.nonce_of(salt, seq), E.ad_of(spi, seq if esn else seq & E.M32, esn)
        ks = R.xor_stream(key, nonce, bytes(n))
        seed = next(f"esp {tname} {n} {G} {esn} {j}" for j in range(10000) if QS.rnd(n, f"lanes esp {tname} {n} {G} {esn} {j}")[n - 2] == ks[n - 2])
        ct, tries, skipped = QS.forge_lanes(key, nonce, ad, n, G, mf.B_TARGETS[tname], seed)
        r, _ = RB.poly_rs(key, nonce)
        H, ts = QM.lane_sums(R.mac_stream(ad, ct), len(ad), n, r, G)
        sets = QM.lane_sets(len(ad), n, G)[:-1]
        alone = [t for t, blocks in sets if blocks == (0,)]  # the lane whose only slot in use is the AD's
        assert skipped == len(alone) == (1 if QM.geom(n, G)[2] % QM.geom(n, G)[1] == 0 else 0)
        assert ts == mf.B_TARGETS[tname] and all(H[t] == mf.B_TARGETS[tname] for t, _ in sets if t not in alone)
        assert QM.tag(key, nonce, ad, ct, G) == R.tag_of(key, nonce, ad, ct)
        pt = R.xor_stream(key, nonce, ct)
        assert pt[n - 2] == 0
        pkts.append(Pkt(pt[:-2], seq, kidx=1, nh=pt[n - 1], iv=seq))
        msgs.append(E.header_of(spi, seq, seq) + ct + R.tag_of(key, nonce, ad, ct))
    case = EspCase(pkts, esn=esn, tops=(2**34 + 9001,) * 4)
    assert [case.protected(i) for i in range(case.count)] == msgs
    o = open_whole(case, msgs, max_len=max_len, where=("lanes", max_len, esn, tname))
    assert o.arrays["status"].got[:case.count].tolist() == [0] * case.count
    seal_whole(case, max_len=max_len - 34, where=("lanes", max_len, esn, tname))


def test_graph_capture(gpu):
    """One seal and one open captured on a single stream and replayed once: the bytes of the
    direct calls."""
    import torch

    from suruga_amd import esp as ESP

    count = 300
    pkts = [Pkt(rnd(1200 - i % 7, f"esp graph {i}"), 2**32 - 100 + 3 * i, kidx=i % 4, nh=NEXT_HEADERS[i % 6]) for i in range(count)]
    case = EspCase(pkts, esn=True, tops=(2**32 + 1000,) * 4, window=2048)
    inp = torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda")
    for o, p in zip(case.raw_off, pkts):
        inp[int(o):int(o) + len(p.payload)] = dev_bytes(p.payload)
    tables = dict(keys=dev_bytes(KEYS4), salts=dev_bytes(SALTS4), spi=dev_u32(SPIS4), sa_index=dev_u32([p.kidx for p in pkts]),
                  esn=True)
    seq, nhs = dev_u64([p.seq for p in pkts]), dev_u8(np.array([p.nh for p in pkts], dtype=np.uint8))
    top = dev_u64(case.tops)
    lens, mlens = dev_u32(case.lens), dev_u32(case.pkt_lens)
    raw_off, msg_off = dev_u64(case.raw_off), dev_u64(case.msg_off)

    def run(ct, back, st, seq_out, plen, nh_out, stream):
        ESP.seal_esp(ESP.EspBatch(count=count, inp=inp, out=ct, status=st[:count], lens=lens, max_len=1300, in_off=raw_off,
                                  out_off=msg_off, seq=seq, next_header=nhs, stream=stream, **tables))
        ESP.open_esp(ESP.EspBatch(count=count, inp=ct, out=back, status=st[count:], seq_out=seq_out, payload_len=plen,
                                  next_header_out=nh_out, replay_top=top, window=2048, lens=mlens, max_len=1300,
                                  in_off=msg_off, out_off=raw_off, stream=stream, **tables))

    def buffers():
        return (torch.zeros(case.msg_size + 16, dtype=torch.uint8, device="cuda"),
                torch.zeros(case.raw_size + 16, dtype=torch.uint8, device="cuda"), filled(2 * count, 0xFF),
                torch.full((count,), -1, dtype=torch.int64, device="cuda"),
                torch.full((count,), -1, dtype=torch.int32, device="cuda"), filled(count, 0xEE))

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
    captured[5].fill_(0xEE)
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(direct, captured):
        assert bool(torch.equal(a, b))
    ct_h, back_h = host_bytes(direct[0]), host_bytes(direct[1])
    assert host_bytes(direct[2]) == bytes(2 * count)
    assert host_np(direct[3]).view(np.uint64).tolist() == [p.seq for p in pkts]
    assert host_np(direct[4]).tolist() == case.lens.tolist()
    assert host_np(direct[5]).tolist() == [p.nh for p in pkts]
    for i in range(0, count, 13):
        lo = int(case.msg_off[i])
        assert ct_h[lo:lo + len(case.protected(i))] == case.protected(i)
        lo = int(case.raw_off[i])
        assert back_h[lo:lo + len(pkts[i].payload)] == pkts[i].payload


def test_round_trip_zipf(gpu):
    """esp.py end to end: 4,096 payloads of Zipf lengths over 7 SAs with extended sequence
    numbers through seal, then open in place; the sequence numbers, the payload lengths, the
    next headers and the payloads come back, and a few packets are the reference's."""
    import torch

    import suruga_amd as S
    from suruga_amd import workloads as WL

    count, sas, align, window = 4096, 7, 4, 8192
    k = WL.zipf_lengths(count) // 64
    lens = np.clip(64 * k - 63 + (13 * np.arange(count)) % 64, 0, 16350).astype(np.uint32)
    mlens = np.array([E.packet_len(int(n), align) for n in lens], dtype=np.uint32)
    assert int(lens.max()) > 2048 and all(S.esp_packet_len(int(n), align) == int(m) for n, m in zip(lens[:64], mlens[:64]))
    slot = (mlens.astype(np.uint64) + np.uint64(15)) // np.uint64(16) * np.uint64(16) + np.uint64(16)
    msg_off = np.concatenate(([0], np.cumsum(slot)[:-1])).astype(np.uint64) + (np.arange(count, dtype=np.uint64) % np.uint64(16))
    size = int(msg_off[-1] + slot[-1]) + 16
    host = np.random.default_rng(7634).integers(0, 256, size=size, dtype=np.uint8)
    keys = b"".join(R.data(32, b"esp sa %d" % j) for j in range(sas))
    salts = b"".join(R.data(4, b"esp sa salt %d" % j) for j in range(sas))
    spis = [0x1000 + j for j in range(sas)]
    kidx = np.arange(count) % sas
    base = [(j + 1) * 2**32 - 3000 for j in range(sas)]  # every SA crosses a 2^32 boundary within the batch
    seqs = [base[int(kidx[i])] + i for i in range(count)]
    tops = [base[j] + count for j in range(sas)]
    nhs = (np.arange(count) * 7 % 256).astype(np.uint8)
    buf = torch.from_numpy(host.copy()).to("cuda")
    st, seq_out, plen, nh_out = filled(count, 0xFF), dev_u64([0] * count), dev_u32([0] * count), filled(count, 0xEE)
    common = dict(count=count, keys=dev_bytes(keys), salts=dev_bytes(salts), spi=dev_u32(spis), sa_index=dev_u32(kidx), status=st,
                  esn=True)
    S.seal_esp(S.EspBatch(inp=buf[16:], out=buf, seq=dev_u64(seqs), next_header=dev_u8(nhs), align=align, lens=dev_u32(lens),
                          max_len=16350, in_off=dev_u64(msg_off), out_off=dev_u64(msg_off), **common))
    torch.cuda.synchronize()
    assert host_bytes(st) == bytes(count)
    sealed = host_np(buf)
    for i in (0, 1, 777, int(np.argmax(lens)), int(np.argmin(lens)), count - 1):
        o, n, j = int(msg_off[i]), int(lens[i]), int(kidx[i])
        want = E.protect(keys[32 * j:32 * j + 32], salts[4 * j:4 * j + 4], spis[j], seqs[i], host[o + 16:o + 16 + n].tobytes(),
                         int(nhs[i]), align=align, esn=True)
        assert sealed[o:o + int(mlens[i])].tobytes() == want, i
    st.fill_(0xFF)
    S.open_esp(S.EspBatch(inp=buf, out=buf[16:], seq_out=seq_out, payload_len=plen, next_header_out=nh_out,
                          replay_top=dev_u64(tops), window=window, lens=dev_u32(mlens), max_len=16384, in_off=dev_u64(msg_off),
                          out_off=dev_u64(msg_off), **common))
    torch.cuda.synchronize()
    assert host_bytes(st) == bytes(count)
    assert host_np(seq_out).view(np.uint64).tolist() == seqs and host_np(plen).view(np.uint32).tolist() == lens.tolist()
    assert host_np(nh_out).tolist() == nhs.tolist()
    back = host_np(buf)
    for i in range(count):
        o, n = int(msg_off[i]) + 16, int(lens[i])
        assert np.array_equal(back[o:o + n], host[o:o + n]), i
        pad = int(mlens[i]) - 32 - n - 2
        assert back[o + n:o + n + pad + 2].tobytes() == E.trailer(pad, int(nhs[i])), i  # the trailer came back in place
