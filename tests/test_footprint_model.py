"""CPU checks of tests/footprint.py: the sentinel, the layouts, the expected
images and the route predicates that the GPU footprint tests rely on
(tests/test_gpu_footprint.py runs exactly these plans)."""
from __future__ import annotations

import numpy as np
import pytest

import footprint as fp

PLANS = {"listed": fp.listed_plan, "packed": fp.packed_plan, "bucket": fp.bucket_plan}


def test_sentinel_has_no_runs_and_no_short_period():
    s = fp.sentinel(1 << 16, 0x35)
    assert s.dtype == np.uint8 and s.size == 1 << 16
    for v in (0x00, 0xEE):  # never twice in a row
        hit = s == v
        assert not (hit[1:] & hit[:-1]).any()
    for period in (1, 2, 4, 8, 16, 32, 64):
        assert (s[period:] != s[:-period]).mean() > 0.99, period
    # moved by 1..16 bytes it differs from itself almost everywhere (only at some 256-byte seams not)
    for k in range(1, 17):
        same = np.flatnonzero(s[k:] == s[:-k])
        assert same.size <= (1 << 16) // 256 * k, k
    # a store of zeros or of a fill byte over any 2 bytes shows
    for v in (0x00, 0xEE, 0xFF):
        for off in range(0, 4096):
            assert (s[off:off + 2] != v).any()
    assert not np.array_equal(fp.sentinel(512, 1), fp.sentinel(512, 2))


def test_image_lays_parts_over_the_sentinel():
    img = fp.image(600, 7, [(256, b"\x01\x02\x03"), (300, b"")])
    want = fp.sentinel(600, 7)
    want[256:259] = (1, 2, 3)
    assert np.array_equal(img, want)
    assert fp.first_diff(img, want) is None
    want[258] ^= 1
    assert "record 0 byte 2 of 3" in fp.first_diff(img, want, [(256, 259)])
    with pytest.raises(AssertionError):
        fp.image(10, 0, [(8, b"abc")])


@pytest.mark.parametrize("align", [1, 16])
def test_layout_margins_gaps_and_alignment(align):
    in_lens = [0, 1, 15, 16, 17, 100, 4096, 5, 64, 63, 1000, 3, 2, 1, 0, 16384, 7, 9, 11, 13, 40]
    out_lens = [n + 16 for n in in_lens]
    in_off, out_off, in_size, out_size = fp.layout(in_lens, out_lens, align=align)
    for off, lens, size in ((in_off, in_lens, in_size), (out_off, out_lens, out_size)):
        assert fp.disjoint(fp.ranges(off, lens), size)
        assert int(off[0]) >= fp.MARGIN and size - (int(off[-1]) + lens[-1]) >= fp.MARGIN
        gaps = fp.gaps_of(off, lens)
        if align == 1:
            assert gaps == [fp.GAPS[i % len(fp.GAPS)] for i in range(len(lens) - 1)]
            assert set(gaps) == set(fp.GAPS)
        else:
            assert all(int(o) % 16 == 0 for o in off)
            # the gap asked for, plus what rounding the next offset up to 16 adds
            assert all(0 <= g - fp.GAPS_ALIGNED[i % 3] < 16 for i, g in enumerate(gaps))
    odd = {2, 5}
    in_off, out_off, _, _ = fp.layout(in_lens, out_lens, odd=odd)
    assert all(int(in_off[i]) % 2 == 1 and int(out_off[i]) % 2 == 1 for i in odd)
    assert not fp.disjoint([(256, 300), (299, 310)], 1000) and not fp.disjoint([(256, 800)], 1000)


def test_route_predicates():
    assert [fp.size_class(n) for n in (0, 128, 129, 256, 257, 8192, 8193, 16384, 32768)] == [0, 0, 1, 1, 2, 6, 7, 7, 7]
    assert [fp.size_class(n) for n in fp.SC_LENGTHS] == list(range(8))
    assert fp.uniform_wpr(16384, False, 0, 0, 16384 + 48, 16400 + 48)
    assert not fp.uniform_wpr(16384, False, 0, 0, 16384 + 8, 16400)       # stride not 16-byte aligned
    assert not fp.uniform_wpr(16384, False, 1, 0, 16384, 16400)           # base
    assert not fp.uniform_wpr(16384, True, 0, 0, 16384, 16400)            # len / offset arrays
    assert not fp.uniform_wpr(16320, False, 0, 0, 16320, 16336)
    assert not fp.uniform_wpr(16384, False, 0, 0, 16384, 16400, lockstep=False)
    assert [fp.bucket_of(n, 0, 16) for n in fp.BUCKET_LENGTHS] == [2, 2, 3, 3, 4, 4]
    assert [fp.bucket_of(n, a, b) for n, a, b in ((4096, 0, 0), (4097, 0, 0), (16448, 0, 0), (8192, 1, 0),
                                                   (8192, 0, 8))] == [0] * 5
    assert all(fp.pack_ok(n, 32, 48) for n in fp.PACKED_LENGTHS)
    assert not any(fp.pack_ok(n, a, b) for n, a, b in ((0, 0, 0), (63, 0, 0), (65, 0, 0), (4160, 0, 0), (64, 4, 0),
                                                        (64, 0, 15)))
    assert fp.mixed_routes(16384, True, True) == (True, True)
    assert fp.mixed_routes(4096, True, True) == (False, True)
    assert fp.mixed_routes(16384, False, True) == (False, False)          # explicit nonce / AD
    assert fp.mixed_routes(16384, True, False) == (False, False)          # uniform
    assert fp.mixed_routes(128, True, True) == (False, False)             # one class: launched directly
    assert fp.mixed_routes(16384, True, True, lockstep=False, packed=False) == (False, False)
    assert fp.mixed_routes(16384, True, True, lockstep=False) == (False, True)
    assert fp.route(8192, 0, 0, True, True) == ("bucket", 2) and fp.route(8192, 0, 0, False, True) == ("class", 6)
    assert fp.route(1024, 0, 0, True, True) == ("packed",) and fp.route(1024, 0, 1, True, True) == ("class", 3)


@pytest.mark.parametrize("name", PLANS)
def test_plans_are_disjoint_and_reach_their_routes(name):
    plan = PLANS[name]()
    aligned = name != "listed"
    for direction in (plan.seal, plan.open):
        in_lens, out_lens, in_off, out_off, in_size, out_size = direction
        assert fp.disjoint(fp.ranges(in_off, in_lens), in_size) and fp.disjoint(fp.ranges(out_off, out_lens), out_size)
        assert out_lens[plan.i_short] > 0 and out_lens[plan.i_long] > plan.max_n  # "untouched" means something
        if aligned:
            assert all(int(o) % 16 == 0 for o in list(in_off) + list(out_off))
            assert set(fp.gaps_of(out_off, out_lens)) >= set(fp.GAPS_ALIGNED)
        else:
            assert set(fp.gaps_of(in_off, in_lens)) >= set(fp.GAPS)
            assert set(fp.gaps_of(out_off, out_lens)) >= set(fp.GAPS)
        counts = plan.routes(direction, True)
        if name == "listed":
            fp.expect_listed_routes(counts, False)
            fp.expect_listed_routes(plan.routes(direction, True, False, False), True)
            fp.expect_listed_routes(plan.routes(direction, False), True)
            # what the packed and bucket kernels would take sits at odd offsets: all of it went to a class
            forced = [i for i in plan.ordinary if plan.all_lens[i] in fp.PACKED_LENGTHS + fp.BUCKET_LENGTHS]
            assert len(forced) >= 3 * 10
            for i in forced:
                assert int(in_off[i]) % 2 == 1 and int(out_off[i]) % 2 == 1
                assert fp.route(plan.all_lens[i], int(in_off[i]), int(out_off[i]), True, True)[0] == "class"
        elif name == "packed":
            fp.expect_packed_routes(counts)
            packed = [plan.all_lens[i] for i in plan.ordinary if plan.all_lens[i] <= 4096]
            assert set(packed) == {64 * k for k in range(1, 65)} and len(packed) == 300 > 2 * 128
        else:
            fp.expect_bucket_routes(counts)
            assert all(plan.all_lens.count(n) >= 4 for n in fp.BUCKET_LENGTHS)


@pytest.mark.parametrize("name", PLANS)
def test_expected_images_leave_the_sentinel_at_every_record_edge(oracle, name):
    """A record whose first or last expected byte equalled the sentinel there would
    hide a one-byte underwrite: the salt is moved until none does, in at most
    MAX_SALT_TRIES tries, for every image the GPU test builds from these plans."""
    plan = PLANS[name]()
    modes = fp.LISTED_MODES if name == "listed" else ("tls",)
    for mode in modes:
        recs = fp.records(oracle, plan.all_lens, mode, fp.PLAN_SEQ0)
        assert sum(fp.is_tampered(i) for i in plan.ordinary) >= plan.count // 7 - 2
        images = fp.plan_images(plan, recs)
        assert [w for w, *_ in images] == ["seal"] + [w for w, _, _ in fp.OPEN_VARIANTS]
        for what, size, parts, salt, tries in images:
            assert tries <= fp.MAX_SALT_TRIES, (mode, what)
            assert len(parts) >= len(plan.ordinary)
            assert fp.edges_differ(size, salt, parts)
            img, bare = fp.image(size, salt, parts), fp.sentinel(size, salt)
            for off, b in parts:
                if len(b):
                    assert img[int(off)] != bare[int(off)] and img[int(off) + len(b) - 1] != bare[int(off) + len(b) - 1]
            # nothing but the parts differs from the sentinel
            mask = np.zeros(size, dtype=bool)
            for off, b in parts:
                mask[int(off):int(off) + len(b)] = True
            assert np.array_equal(img[~mask], bare[~mask])
