"""The Python model of the TLS 1.3 read's gather step (record13_ref.gather_model)
and its checker (gather_check), which the GPU tests hold sg_gather_kernel
against: the prefix, ``ok``, the cursor chain and the sticky stop, and the checker
failing on wrong images.  CPU only."""
from __future__ import annotations

import numpy as np
import pytest

import footprint as fp
import record13_ref as RR

STRIDE = 64


def _src(count, salt=3):
    return fp.sentinel(count * STRIDE, salt) ^ np.uint8(0x5A)


def _run(status, lens, cur=None, use_base=False, dst_off=5, size=400):
    src = _src(len(lens))
    dst = fp.sentinel(size, 9)
    return src, dst, RR.gather_model(src, STRIDE, status, lens, dst, dst_off, cur or RR.Cursor(), use_base)


def test_prefix_and_ok_with_empty_records():
    lens = [3, 0, 0, 5, 1, 0, 4]
    src, dst, (img, cur, res) = _run([0] * 7, lens)
    assert res == (7, 13) and (cur.offset, cur.stopped) == (13, 0)
    want = b"".join(src[i * STRIDE:i * STRIDE + n].tobytes() for i, n in enumerate(lens))
    assert img[5:18].tobytes() == want
    assert np.array_equal(img[:5], dst[:5]) and np.array_equal(img[18:], dst[18:])


@pytest.mark.parametrize("bad,ok,total", [(0, 0, 0), (2, 2, 8), (3, 3, 8 + 7)])
def test_first_failing_status_stops(bad, ok, total):
    lens, status = [4, 4, 7, 9], [0, 0, 0, 0]
    status[bad] = 1
    src, dst, (img, cur, res) = _run(status, lens)
    assert res == (ok, total) and (cur.offset, cur.stopped) == (total, 1)
    assert np.array_equal(img[5 + total:], dst[5 + total:])  # nothing from the failing record on


def test_content_above_2_14_stops_like_a_status():
    _, _, (_, cur, res) = _run([0, 0], [2, RR.FULL + 1])
    assert res == (1, 2) and cur.stopped == 1
    _, _, (_, cur, res) = _run([0, 5], [2, 0])  # SG_STATUS_NO_TYPE
    assert res == (1, 2) and cur.stopped == 1


def test_sticky_stop_and_chain():
    src, dst, (img, cur, res) = _run([0, 0], [6, 2], RR.Cursor(40, 1), use_base=True)
    assert res == (0, 0) and (cur.offset, cur.stopped) == (40, 1) and np.array_equal(img, dst)
    # two chained chunks: the second lands at the first one's end
    src, dst, (img1, c1, r1) = _run([0, 0], [6, 2], RR.Cursor(), use_base=True)
    img2, c2, r2 = RR.gather_model(src, STRIDE, [0, 1], [3, 9], img1, 5, c1, True)
    assert (c1.offset, c2.offset, c2.stopped, r2) == (8, 11, 1, (1, 3))
    assert img2[5 + 8:5 + 11].tobytes() == src[:3].tobytes()
    # without use_base the chunk lands at the destination's start, the cursor still runs
    img3, c3, _ = RR.gather_model(src, STRIDE, [0], [3], dst, 5, RR.Cursor(100, 0), False)
    assert c3.offset == 103 and img3[5:8].tobytes() == src[:3].tobytes()


def test_checker_fails_on_wrong_images():
    src, dst, (img, cur, res) = _run([0, 0, 1], [5, 6, 7])
    RR.gather_check(img.copy(), (cur.offset, cur.stopped), res, img, cur, res)
    for mutate in (lambda a: a.__setitem__(5 + 11, a[5 + 11] ^ 1),       # a byte of the failing record delivered
                   lambda a: a.__setitem__(4, 0),                         # a store in front of dst
                   lambda a: a.__setitem__(slice(5, 16), np.roll(a[5:16], 1)),  # shifted by one byte
                   lambda a: a.__setitem__(5 + 10, dst[5 + 10])):         # the last byte not written
        bad = img.copy()
        mutate(bad)
        with pytest.raises(AssertionError):
            RR.gather_check(bad, (cur.offset, cur.stopped), res, img, cur, res)
    with pytest.raises(AssertionError):
        RR.gather_check(img.copy(), (cur.offset, 0), res, img, cur, res)  # the stop not handed on
    with pytest.raises(AssertionError):
        RR.gather_check(img.copy(), (cur.offset, cur.stopped), (3, res[1]), img, cur, res)
