"""Input generator for the adversarial Poly1305 tests (tests/test_mac_forge.py on
the CPU, tests/test_gpu_mac_edges.py on the GPU) -- TEST INFRASTRUCTURE ONLY.

The MAC of a record runs over its ciphertext, so ciphertext can be chosen that
drives the Poly1305 accumulator, or any partial sum of it, to a chosen value:
the states a random record reaches with probability 2^-96 or less.  For one
record's key and nonce, keystream block 0 gives r (clamped) and s; the MAC
stream is ad || le64(|ad|) || ct || le64(n) (chacha20_poly1305.rs:19-42),
block i has the value c_i = its bytes little-endian + 2^(8 len), B blocks in
all, and the accumulator before s is sum_i c_i r^(B - i) mod p.

A constraint (blocks, E, T) demands sum_{i in blocks} c_i r^(E - i) == T
(mod p).  It is solved by one block of the set that lies wholly inside ct:
c = (T - rest) r^-(E - b) mod p is a block value when c - 2^128 is in
[0, 2^128), about one try in four; otherwise another block's ciphertext bytes
are drawn again from the seeded generator.  The tag is then computed by an
independent Horner pass.  Nothing here is the reference: the tests compare
every forged record with oracle.seal / oracle.open.

The second half of the module lists the records both test files use, one
function per finishing path of the library, so that the CPU test checks exactly
the inputs the GPU test feeds the kernels.  Records are cached per shape.
"""
from __future__ import annotations

import functools
import hashlib
import struct
from dataclasses import dataclass, field

import numpy as np

import wpr_model

P = (1 << 130) - 5
CLAMP = 0x0FFFFFFC0FFFFFFC0FFFFFFC0FFFFFFF
M128 = (1 << 128) - 1
KEY = bytes(range(32))
MAX_TRIES = 1000  # the tests hold every solve to 200


def _oracle():
    from oracle_ffi import oracle

    return oracle()


def poly_key(key: bytes, nonce: bytes):
    """(r, s) of one record: keystream block 0 (chacha20_poly1305.rs:50, poly1305.rs:197-203)."""
    ks = _oracle().keystream(key, nonce, 64)
    return int.from_bytes(ks[:16], "little") & CLAMP, int.from_bytes(ks[16:32], "little")


def mac_stream(ad: bytes, ct: bytes) -> bytes:
    """chacha20_poly1305.rs:19-42: ad || le64(|ad|) || ct || le64(|ct|), no padding."""
    return bytes(ad) + struct.pack("<Q", len(ad)) + bytes(ct) + struct.pack("<Q", len(ct))


def n_blocks(adlen: int, n: int) -> int:
    return (adlen + 16 + n + 15) // 16


def block_value(stream, i: int) -> int:
    chunk = stream[16 * i:16 * i + 16]
    return int.from_bytes(chunk, "little") + (1 << (8 * len(chunk)))


def horner_tag(stream: bytes, r: int, s: int) -> bytes:
    """poly1305.rs:207-312, sequentially."""
    h = 0
    for i in range((len(stream) + 15) // 16):
        h = (h + block_value(stream, i)) * r % P
    return ((h + s) & M128).to_bytes(16, "little")


def _target(T, r, s, stream) -> int:
    return (T(r, s, stream) if callable(T) else T) % P


@dataclass
class Forged:
    key: bytes
    nonce: bytes
    ad: bytes
    ct: bytes
    tag: bytes
    pt: bytes
    r: int
    s: int
    constraints: list            # as given: (blocks, E, T)
    skipped: list                # indices of constraints whose set holds no full ciphertext block
    tries: dict                  # constraint index -> tries of its solve
    seq: int | None = None       # TLS mode: the record's sequence number
    want: bytes = b""            # oracle.seal of pt (filled in by make())
    case: tuple = field(default=())

    def __iter__(self):
        return iter((self.ct, self.tag, self.pt))

    def stream(self) -> bytes:
        return mac_stream(self.ad, self.ct)

    def partial(self, idx: int):
        """(sum_{i in blocks} c_i r^(E - i) mod p, T mod p) of constraint idx, recomputed from the final bytes."""
        blocks, E, T = self.constraints[idx]
        st = self.stream()
        lhs = sum(block_value(st, i) * pow(self.r, E - i, P) for i in blocks) % P
        return lhs, _target(T, self.r, self.s, st)

    def accumulator(self) -> int:
        """The whole-stream accumulator before s, mod p."""
        st, h = self.stream(), 0
        for i in range((len(st) + 15) // 16):
            h = (h + block_value(st, i)) * self.r % P
        return h


def forge_report(key: bytes, nonce: bytes, ad: bytes, n: int, constraints, seed: int, ct: bytes | None = None) -> Forged:
    """Forge one record.  constraints: (blocks, E, T) with disjoint block sets; T
    an integer or a function of (r, s, stream) that reads only stream bytes
    outside every constraint's set.  ct: the ciphertext to start from (default:
    n bytes of default_rng(seed))."""
    orc = _oracle()
    ks = orc.keystream(key, nonce, 64 + n)
    r = int.from_bytes(ks[:16], "little") & CLAMP
    s = int.from_bytes(ks[16:32], "little")
    rng = np.random.default_rng(seed)
    off, adlen = len(ad) + 8, len(ad)
    stream = bytearray(mac_stream(ad, rng.bytes(n) if ct is None else ct))
    assert len(stream) == adlen + 16 + n
    B = n_blocks(adlen, n)
    constraints = [(tuple(sorted(b)), E, T) for b, E, T in constraints]
    seen: set = set()
    for blocks, E, _ in constraints:
        assert blocks and not seen.intersection(blocks) and blocks[0] >= 0 and blocks[-1] < B and E > blocks[-1]
        seen.update(blocks)
    rp = [1]
    for _ in range(max([E for _, E, _ in constraints], default=0)):
        rp.append(rp[-1] * r % P)
    skipped, tries = [], {}
    for idx, (blocks, E, T) in enumerate(constraints):
        full = [b for b in blocks if 16 * b >= off and 16 * b + 16 <= off + n]
        if not full:
            skipped.append(idx)
            continue
        free = full[-1]
        # blocks of the set, other than the free one, that hold ciphertext bytes
        redraw = [b for b in blocks if b != free and 16 * b + 16 > off and 16 * b < off + n]
        want = _target(T, r, s, stream)
        rest = sum(block_value(stream, i) * rp[E - i] for i in blocks if i != free) % P
        inv = pow(rp[E - free], -1, P)
        for t in range(1, MAX_TRIES + 1):
            c = (want - rest) * inv % P
            if (1 << 128) <= c < (1 << 129):
                stream[16 * free:16 * free + 16] = (c - (1 << 128)).to_bytes(16, "little")
                tries[idx] = t
                break
            if not redraw:
                raise RuntimeError(f"constraint {idx}: one ciphertext block and nothing to draw again")
            b = redraw[int(rng.integers(len(redraw)))]
            lo, hi = max(16 * b, off), min(16 * b + 16, off + n)
            old = block_value(stream, b)
            stream[lo:hi] = rng.bytes(hi - lo)
            rest = (rest + (block_value(stream, b) - old) * rp[E - b]) % P
        else:
            raise RuntimeError(f"constraint {idx}: no solution in {MAX_TRIES} tries")
    ct_out = bytes(stream[off:off + n])
    pt = bytes(np.frombuffer(ct_out, dtype=np.uint8) ^ np.frombuffer(ks, dtype=np.uint8)[64:64 + n]) if n else b""
    return Forged(key=key, nonce=nonce, ad=bytes(ad), ct=ct_out, tag=horner_tag(bytes(stream), r, s), pt=pt, r=r, s=s,
                  constraints=constraints, skipped=skipped, tries=tries)


def forge(key: bytes, nonce: bytes, ad: bytes, n: int, constraints, seed: int):
    """(ct, tag, pt) of forge_report."""
    f = forge_report(key, nonce, ad, n, constraints, seed)
    return f.ct, f.tag, f.pt


# ---------------------------------------------------------------------------
# Tier A: targets of the final accumulator, functions of (r, s)
# ---------------------------------------------------------------------------
X128 = 0x0F1E2D3C4B5A69788796A5B4C3D2E1F0  # "one fixed x", below 2^128 - 5


def _tag00(k):
    return lambda r, s, st: ((-s) & M128) + (k << 128)  # low 128 bits -s: every w_i + s_i carries


TARGETS = {str(v): v for v in (0, 1, 2, 3, 4, 5, 6, 63, 64, 255, 319, 320)}
TARGETS.update({f"p-{d}": P - d for d in (1, 2, 3, 4, 5)})
TARGETS.update({"2^128-1": (1 << 128) - 1, "2^128": 1 << 128, "2^129": 1 << 129})
TARGETS.update({f"x+{k}*2^128": X128 + (k << 128) for k in range(4)})
TARGETS.update({f"tag00+{k}*2^128": _tag00(k) for k in range(4)})
TARGETS["tagff"] = lambda r, s, st: (-s - 1) & M128  # low 128 bits -s-1: no carry anywhere
TAG_PATTERN = {**{f"tag00+{k}*2^128": bytes(16) for k in range(4)}, "tagff": b"\xff" * 16}
# (target, seed): four seeds for the targets 0..4, one for the rest
A_CASES = [(name, seed) for name in TARGETS for seed in range(4 if name in ("0", "1", "2", "3", "4") else 1)]
B_TARGETS = {"m1": P - 1, "zero": 0}  # Tier B: every term == -1 (all limbs at their maximum), every term == 0


# ---------------------------------------------------------------------------
# the kernels' partitions of the MAC stream
# ---------------------------------------------------------------------------
def size_class(n: int) -> int:
    """sg_internal.h size_class: class c holds n <= 128 << c, class 7 the rest."""
    return 0 if n <= 128 else min(7, ((n - 1) >> 7).bit_length())


def sizeclass_geom(adlen: int, n: int):
    """sg_kernels.hip mac_geom: (PL, B, k, z)."""
    PL = min(2 << size_class(n), 64)
    B = n_blocks(adlen, n)
    k = -(-B // PL) | 1
    return PL, B, k, PL * k - B


def sizeclass_lanes(adlen: int, n: int):
    """Real blocks of every MAC lane that has some: lane t owns [t k - z, (t + 1) k - z) within [0, B)."""
    PL, B, k, z = sizeclass_geom(adlen, n)
    sets = [range(max(0, t * k - z), min(B, (t + 1) * k - z)) for t in range(PL)]
    return [tuple(x) for x in sets if len(x)]


def fewest_virtual(cls: int, adlen: int) -> int:
    """The smallest length of size class cls whose geometry leaves the fewest lanes
    without a real block (z / k of them), among those with k >= 3 blocks a lane
    (class 0 from 65 bytes on, so that the lanes hold whole ciphertext blocks)."""
    lo = 65 if cls == 0 else (128 << (cls - 1)) + 1
    geoms = {n: sizeclass_geom(adlen, n) for n in range(lo, (128 << cls) + 1)}
    return min((n for n, g in geoms.items() if g[2] >= 3), key=lambda n: (geoms[n][3] // geoms[n][2], n))


def packed_lane_term(stream: bytes, r: int, n: int, j: int) -> int:
    """sg_pack.hip: the share of lane j (ciphertext bytes 64 j .. 64 j + 63 of a TLS
    record) -- its bytes at their stream positions 21 + 64 j .. and the 2^128
    pads of blocks 4 j + 1 .. 4 j + 4 -- in the accumulator, mod p."""
    B = 4 * (n // 64) + 2
    total = 0
    for b in range(4 * j + 1, 4 * j + 6):
        lo, hi = max(16 * b, 21 + 64 * j), min(16 * b + 16, 21 + 64 * j + 64)
        v = int.from_bytes(stream[lo:hi], "little") << (8 * (lo - 16 * b))
        if b < 4 * j + 5:
            v += 1 << 128
        total += v * pow(r, B - b, P)
    return total % P


def packed_constraints(n: int, target: int):
    """Lane j's term == target, as a constraint on its three whole blocks
    4 j + 2 .. 4 j + 4: the lane's bytes in blocks 4 j + 1 and 4 j + 5 (which
    belong to no set and are never redrawn) and the pad of 4 j + 1 fold into T."""
    assert n % 64 == 0 and 64 <= n <= 4096
    B = 4 * (n // 64) + 2
    out = []
    for j in range(n // 64):
        def T(r, s, st, j=j):
            a = (int.from_bytes(st[16 * (4 * j + 1) + 5:16 * (4 * j + 2)], "little") << 40) + (1 << 128)
            b = int.from_bytes(st[16 * (4 * j + 5):16 * (4 * j + 5) + 5], "little")
            return target - a * pow(r, B - 4 * j - 1, P) - b * pow(r, B - 4 * j - 5, P)
        out.append(((4 * j + 2, 4 * j + 3, 4 * j + 4), B, T))
    return out


def msg_plan(n: int, adlen: int, groups: int) -> dict:
    from suruga_amd import msg

    return msg.plan_for(n, adlen, groups)


def msg_lane_sets(plan: dict):
    """sg_msg.hip: lane l of a group keeps blocks 4 l .. 4 l + 3 of every tile of
    the group; (blocks, E) with E just past the group's last tile (real indices)."""
    K, z, T, per = plan["tile_blocks"], plan["zero_blocks"], plan["tiles"], plan["tiles_per_group"]
    out = []
    for g in range(plan["groups"]):
        lo, hi = g * per, min(T, (g + 1) * per)
        for l in range(K // 4):
            blocks = tuple(t * K + 4 * l + j - z for t in range(lo, hi) for j in range(4) if t * K + 4 * l + j >= z)
            if blocks:
                out.append((blocks, hi * K - z))
    return out


def msg_group_sets(plan: dict):
    """Each group's whole block set, E = B: its partial at its place in the finish kernel's sum."""
    K, z, T, per = plan["tile_blocks"], plan["zero_blocks"], plan["tiles"], plan["tiles_per_group"]
    out = []
    for g in range(plan["groups"]):
        lo, hi = g * per, min(T, (g + 1) * per)
        out.append((tuple(range(max(0, lo * K - z), hi * K - z)), plan["mac_blocks"]))
    return out


def tile_bytes() -> int:
    return msg_plan(0, 0, 0)["tile_bytes"]


# ---------------------------------------------------------------------------
# Tier C: ciphertext against the wave-per-record kernel's i8 MFMA accumulators
# ---------------------------------------------------------------------------
FILLS = {"00": b"\x00", "7f": b"\x7f", "80": b"\x80", "ff": b"\xff", "00ff": b"\x00\xff", "ff00": b"\xff\x00"}
SIGN_ROWS = (0, 15, 16, 31)


def wpr_sign_ct(ad: bytes, r: int, row: int, negate: bool) -> bytes:
    """16 KiB of ciphertext whose every byte is 0xff where the signed digit it
    multiplies in accumulator row `row` is >= 0 and 0x00 where it is negative
    (negate: the other way round): |D[row][q]| as large as ciphertext can make
    it.  The T operand is the one tests/wpr_model.py's wpr_tag multiplies by."""
    kt = wpr_model.keying(wpr_model.DRAFT, ad, r)
    lines = wpr_model.digit_lines(kt)
    ct = np.zeros((1024, 16), dtype=np.uint8)
    for j, i, h in wpr_model.STEPS:
        t, m = wpr_model.t_operand(lines, kt["sig"], j, i, h, rows=(row,))
        ct[m] = np.where((t[0] >= 0) != negate, 0xFF, 0x00).astype(np.uint8)
    return ct.tobytes()


# ---------------------------------------------------------------------------
# records, cached per shape
# ---------------------------------------------------------------------------
def _identity(mode, n: int, kind: tuple, seed: int):
    """(nonce, ad, seq, generator seed) of a record: TLS mode ("tls") takes both
    from a sequence number, explicit mode (mode = the AD length) draws them."""
    h = hashlib.shake_256(repr((mode, n, kind, seed)).encode()).digest(16 + 255)
    gen = int.from_bytes(h[8:16], "little")
    if mode == "tls":
        seq = int.from_bytes(h[:8], "little")
        return struct.pack(">Q", seq), _oracle().tls_ad(seq, n), seq, gen
    return h[:8], h[16:16 + mode], None, gen


@functools.lru_cache(maxsize=None)
def make(mode, n: int, kind: tuple, seed: int = 0) -> Forged:
    """The record of one case.  kind:
      ("A", target)            whole-record accumulator == TARGETS[target]
      ("sc", t)                every size-class lane term == B_TARGETS[t]
      ("pk", t)                every packed-kernel lane term
      ("ml", groups, t)        every long-message lane term, grid setting `groups`
      ("mg", groups, t)        every long-message group partial
      ("fill", name)           constant-fill ciphertext FILLS[name]
      ("sign", row, negate)    wpr_sign_ct"""
    nonce, ad, seq, gen = _identity(mode, n, kind, seed)
    adlen, B, ct = len(ad), n_blocks(len(ad), n), None
    if kind[0] == "A":
        cons = [(range(B), B, TARGETS[kind[1]])]
    elif kind[0] == "sc":
        cons = [(b, B, B_TARGETS[kind[1]]) for b in sizeclass_lanes(adlen, n)]
    elif kind[0] == "pk":
        assert mode == "tls"
        cons = packed_constraints(n, B_TARGETS[kind[1]])
    elif kind[0] in ("ml", "mg"):
        sets = (msg_lane_sets if kind[0] == "ml" else msg_group_sets)(msg_plan(n, adlen, kind[1]))
        cons = [(b, E, B_TARGETS[kind[2]]) for b, E in sets]
    elif kind[0] == "fill":
        cons, ct = [], (FILLS[kind[1]] * n)[:n]
    elif kind[0] == "sign":
        assert n == 16384
        cons, ct = [], wpr_sign_ct(ad, poly_key(KEY, nonce)[0], kind[1], kind[2])
    else:
        raise ValueError(kind)
    f = forge_report(KEY, nonce, ad, n, cons, gen, ct=ct)
    f.seq, f.case = seq, (mode, n, kind, seed)
    f.want = _oracle().seal(KEY, nonce, f.pt, ad)
    return f


def tier_a(mode, n: int):
    return [(mode, n, ("A", name), seed) for name, seed in A_CASES]


# the smallest shapes that select each finishing path
SC_LENGTHS = (100, 200, 400, 800, 1600, 3200, 6400, 12800)  # one per size class: PL = 2 .. 64, 64, 64
SC_MODES = ("tls", 0, 29)
WPR_N = 16384
WPR_MODES = ("tls", 0, 7, 255)
BUCKET_LENGTHS = (4160, 8192, 8256, 12288, 12352, 16384)  # first and last length of J = 2, 3, 4
PACKED_LENGTHS = (64, 128, 1024, 4096)
PACKED_B_LENGTHS = (64, 2048, 4096)
MSG_ADLEN = 13
MSG_GROUPS_B = (1, 3, 0)
TRAIT_N = 1000
FILL_OTHER = (("tls", 4096), ("tls", 3200))  # the fills through the packed kernel and a size class


def msg_lengths():
    T = tile_bytes()
    return [total - MSG_ADLEN - 16 for total in (T - 1, T + 1, 3 * T + 5)]


def sizeclass_a():
    """(mode, n) -> cases; n = 16384 runs with the wave-per-record kernel switched off."""
    return {(m, n): tier_a(m, n) for n in SC_LENGTHS + (WPR_N,) for m in SC_MODES}


def wpr_a():
    return {(m, WPR_N): tier_a(m, WPR_N) for m in WPR_MODES}


def bucket_a():
    return [c for n in BUCKET_LENGTHS for c in tier_a("tls", n)]


def packed_a():
    return [c for n in PACKED_LENGTHS for c in tier_a("tls", n)]


def msg_a():
    return {n: tier_a(MSG_ADLEN, n) for n in msg_lengths()}


def trait_a():
    return tier_a(MSG_ADLEN, TRAIT_N)


def sizeclass_b():
    out = {}
    for m in SC_MODES:
        adlen = 13 if m == "tls" else m
        for n in sorted(set(SC_LENGTHS) | {fewest_virtual(c, adlen) for c in range(6)}):
            out[(m, n)] = [(m, n, ("sc", t), seed) for t in B_TARGETS for seed in range(2)]
    return out


def packed_b():
    return [("tls", n, ("pk", t), seed) for n in PACKED_B_LENGTHS for t in B_TARGETS for seed in range(2)]


def msg_b():
    """groups setting -> cases at 3 T + 5 stream bytes."""
    n = msg_lengths()[-1]
    return {g: [(MSG_ADLEN, n, (k, g, t), 0) for k in ("ml", "mg") for t in B_TARGETS] for g in MSG_GROUPS_B}


def wpr_c():
    fills = [("tls", WPR_N, ("fill", name), 0) for name in FILLS]
    signs = [("tls", WPR_N, ("sign", row, neg), 0) for row in SIGN_ROWS for neg in (False, True)]
    return fills + signs


def fills_other():
    return {(m, n): [(m, n, ("fill", name), 0) for name in FILLS] for m, n in FILL_OTHER}


GROUP_NAMES = ("sizeclass_a", "wpr_a", "bucket_a", "packed_a", "msg_a", "trait_a", "sizeclass_b", "packed_b", "msg_b",
               "wpr_c", "fills_other")


def groups_of_cases() -> dict:
    """Every case of the GPU file, by group (the CPU test's parameters)."""
    flat = lambda d: [c for v in d.values() for c in v]
    return {"sizeclass_a": flat(sizeclass_a()), "wpr_a": flat(wpr_a()), "bucket_a": bucket_a(), "packed_a": packed_a(),
            "msg_a": flat(msg_a()), "trait_a": trait_a(), "sizeclass_b": flat(sizeclass_b()), "packed_b": packed_b(),
            "msg_b": flat(msg_b()), "wpr_c": wpr_c(), "fills_other": flat(fills_other())}
