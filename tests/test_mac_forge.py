"""CPU check of tests/mac_forge.py: every record tests/test_gpu_mac_edges.py
feeds the kernels, against the oracle.  The oracle is the ground truth; the
forger only generates inputs.  For every record:

* oracle.seal(key, nonce, pt, ad) == ct || tag and oracle.open gives status 0
  and pt;
* every constraint's congruence holds when recomputed from the final bytes
  (for the packed kernel also in the kernel's own terms: the lane's 64 bytes at
  their stream positions plus its four pads);
* the stated tag patterns (00..00, ff..ff) are hit exactly;
* at most 2 constraints of a record are skipped (the lane or tile holding only
  the AD prefix, the one holding only le64(n)) and no solve took more than 200
  tries: conditions, not measurements.
"""
from __future__ import annotations

import functools

import pytest

import mac_forge as F
import wpr_model as W


@functools.lru_cache(maxsize=None)
def groups() -> dict:
    return F.groups_of_cases()  # not at import: the long-message plan comes from the native library


def check_record(oracle, case):
    f = F.make(*case)
    mode, n, kind, _ = case
    assert len(f.ct) == n and len(f.pt) == n and len(f.ad) == (13 if mode == "tls" else mode), case
    assert oracle.seal(f.key, f.nonce, f.pt, f.ad) == f.ct + f.tag == f.want, case
    assert oracle.open(f.key, f.nonce, f.ct + f.tag, f.ad) == (0, f.pt), case
    assert len(f.skipped) <= 2, (case, f.skipped)
    # ... and they are the set in front of the first whole ciphertext block and the one behind the last
    off = len(f.ad) + 8
    first_full, last_full = -(-off // 16), (off + n) // 16 - 1
    sides = [("front" if f.constraints[i][0][-1] < first_full else "behind" if f.constraints[i][0][0] > last_full
              else "inside") for i in f.skipped]
    assert "inside" not in sides and len(set(sides)) == len(sides), (case, sides)
    assert max(f.tries.values(), default=0) <= 200, case
    assert len(f.tries) + len(f.skipped) == len(f.constraints), case
    for idx in range(len(f.constraints)):
        if idx not in f.skipped:
            lhs, rhs = f.partial(idx)
            assert lhs == rhs, (case, idx)
    if kind[0] == "A":
        assert len(f.constraints) == 1 and not f.skipped, case
        T = F.TARGETS[kind[1]]
        want = (T(f.r, f.s, None) if callable(T) else T)
        assert want < F.P and f.accumulator() == want, case
        if kind[1] in F.TAG_PATTERN:
            assert f.tag == F.TAG_PATTERN[kind[1]], case
    elif kind[0] in ("sc", "pk", "ml", "mg"):
        assert f.constraints, case
    if kind[0] == "pk":
        st = f.stream()
        for j in range(n // 64):
            assert F.packed_lane_term(st, f.r, n, j) == F.B_TARGETS[kind[1]], (case, j)
    return f


@pytest.mark.parametrize("group", [g for g in F.GROUP_NAMES if g != "wpr_c"])
def test_forged_records_against_the_oracle(oracle, group):
    assert set(groups()) == set(F.GROUP_NAMES) and groups()[group]
    for case in groups()[group]:
        check_record(oracle, case)


def test_wpr_extreme_ciphertext_in_the_model(oracle):
    """Tier C: the fills and the sign-aligned patterns keep the model's seeded
    accumulator in (0, 2^25) (asserted inside wpr_tag) and give the oracle's tag."""
    for case in groups()["wpr_c"]:
        f = check_record(oracle, case)
        assert W.wpr_tag(f.ad, f.ct, f.r, f.s, W.keying(W.DRAFT, f.ad, f.r)) == f.tag, case


def test_sign_patterns_follow_the_digit_signs(oracle):
    """A sign-aligned pattern and its negation are complements, hold only 00 and
    ff, and differ between accumulator rows."""
    cts = {}
    cts_ad, cts_r = bytes(13), F.poly_key(F.KEY, bytes(8))[0]  # one record's r for the comparison between rows
    for row in F.SIGN_ROWS:
        f = F.make("tls", F.WPR_N, ("sign", row, False), 0)
        # (row 31 multiplies only the top digit, which is never negative: one value)
        assert set(f.ct) | set(F.make("tls", F.WPR_N, ("sign", row, True), 0).ct) == {0x00, 0xFF}
        assert bytes(x ^ 0xFF for x in f.ct) == F.wpr_sign_ct(f.ad, f.r, row, True)
        cts[row] = F.wpr_sign_ct(cts_ad, cts_r, row, False)
    assert len(set(cts.values())) == len(F.SIGN_ROWS)


def test_every_tier_a_shape_has_every_target():
    names = set(F.TARGETS)
    for cases in list(F.sizeclass_a().values()) + list(F.wpr_a().values()) + list(F.msg_a().values()) + [F.trait_a()]:
        assert {c[2][1] for c in cases} == names
        assert sum(1 for c in cases if c[2][1] == "0") >= 4  # seeds of the targets 0..4
    for n in F.BUCKET_LENGTHS:
        assert {c[2][1] for c in F.bucket_a() if c[1] == n} == names
    for n in F.PACKED_LENGTHS:
        assert {c[2][1] for c in F.packed_a() if c[1] == n} == names
    assert len(F.packed_a()) > 128  # two runs of the packed list


def test_partitions_cover_the_stream():
    """The lane and group sets are partitions of the record's blocks."""
    for (mode, n) in F.sizeclass_b():
        adlen = 13 if mode == "tls" else mode
        PL, B, k, z = F.sizeclass_geom(adlen, n)
        lanes = F.sizeclass_lanes(adlen, n)
        assert sorted(b for lane in lanes for b in lane) == list(range(B)) and len(lanes) == PL - z // k
    assert [F.sizeclass_geom(13, n)[0] for n in F.SC_LENGTHS] == [2, 4, 8, 16, 32, 64, 64, 64]
    n = F.msg_lengths()[-1]
    for g in F.MSG_GROUPS_B:
        plan = F.msg_plan(n, F.MSG_ADLEN, g)
        for sets in (F.msg_lane_sets(plan), F.msg_group_sets(plan)):
            assert sorted(b for blocks, _ in sets for b in blocks) == list(range(plan["mac_blocks"]))
        assert F.msg_group_sets(plan)[-1][1] == F.msg_lane_sets(plan)[-1][1] == plan["mac_blocks"]


def test_a_set_without_a_full_ciphertext_block_is_reported(oracle):
    # adlen 13, n = 40: block 0 is AD || le64, block 1 starts with le64's rest, block 4 holds le64(n)
    f = F.forge_report(F.KEY, bytes(8), bytes(13), 40, [((0,), 5, 7), ((1, 2), 5, 9), ((4,), 5, 11)], seed=1)
    assert f.skipped == [0, 2] and list(f.tries) == [1]
    assert f.partial(1) == (9, 9)
    assert oracle.seal(f.key, f.nonce, f.pt, f.ad) == f.ct + f.tag
    ct, tag, pt = F.forge(F.KEY, bytes(8), bytes(13), 40, [((1, 2), 5, 9)], seed=1)
    assert oracle.open(F.KEY, bytes(8), ct + tag, bytes(13)) == (0, pt)
