"""sg_gather_kernel alone (through sg_gather_records) against the Python model of
record13_ref: counts 1, 2, 255 and 256, lengths from 0 to 2^14, every destination
alignment, a failing status at the first, a middle and the last index, a stopped
incoming cursor and two chained chunks -- whole-buffer comparison on sentinel
buffers, cursor and result included."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import footprint as fp
import record13_ref as RR

pytestmark = pytest.mark.gpu
STRIDE = 18432
FULL = RR.FULL
LENS = (0, 1, 3, 4, 5, FULL, 2, 0, 0, 7, 8, 9, 15, 16, 17, 4095, 4096, 4097, 63, 64, 65, 1000, 11, 6)


def _lens(count):
    return [LENS[i % len(LENS)] for i in range(count)]


def _gather(lib, src_h, status, lens, dst_h, dst_off, cur: RR.Cursor, use_base):
    """One sg_gather_records call -> (dst image, (offset, stopped), (ok, bytes))."""
    import torch

    from gpu_support import dev_u32
    from suruga_amd import _native as N

    count = len(lens)
    d_src = torch.from_numpy(src_h).to("cuda")
    d_dst = torch.from_numpy(dst_h).to("cuda")
    assert d_src.data_ptr() % 16 == 0 and d_dst.data_ptr() % 16 == 0
    d_st = torch.from_numpy(np.array(status, dtype=np.uint8)).to("cuda")
    d_len = dev_u32(lens)
    cur_h = np.array([cur.offset, cur.stopped, 0x7777777777777777, 0x7777777777777777], dtype=np.uint64)
    cur_h[1] = cur.stopped  # {u64 offset, u32 stopped, u32 pad} twice; the second entry starts as a marker
    d_cur = torch.from_numpy(cur_h.view(np.int64)).to("cuda")
    d_res = dev_u32([0xEEEEEEEE, 0xEEEEEEEE, 0xEEEEEEEE])
    N.check(lib.sg_gather_records(d_src.data_ptr(), STRIDE, d_st.data_ptr(), d_len.data_ptr(), count,
                                  d_dst.data_ptr() + dst_off, int(use_base), d_cur.data_ptr(), d_cur.data_ptr() + 16,
                                  d_res.data_ptr(), None))
    torch.cuda.synchronize()
    c = d_cur.cpu().numpy().view(np.uint64)
    assert (int(c[0]), int(c[1])) == (cur.offset, cur.stopped), "the incoming cursor was written"
    r = d_res.cpu().numpy().view(np.uint32)
    assert int(r[2]) == 0xEEEEEEEE
    assert np.array_equal(d_src.cpu().numpy(), src_h), "the source was written"
    return d_dst.cpu().numpy(), (int(c[2]), int(c[3]) & 0xFFFFFFFF), (int(r[0]), int(r[1]))


def _case(lib, count, bad, dst_off, cur=None, use_base=False, lens=None, status=None):
    lens = _lens(count) if lens is None else lens
    status = [0] * count if status is None else list(status)
    if bad is not None:
        status[bad] = 1
    src = fp.sentinel(count * STRIDE, 0x17) ^ np.uint8(0xA5)
    cur = cur or RR.Cursor()
    size = 512 + sum(lens) + (cur.offset if use_base else 0)
    dst = fp.sentinel(size, 0x3C)
    want = RR.gather_model(src, STRIDE, status, lens, dst, 256 + dst_off, cur, use_base)
    got = _gather(lib, src, status, lens, dst, 256 + dst_off, cur, use_base)
    RR.gather_check(got[0], got[1], got[2], *want)
    return want


@pytest.mark.parametrize("align", [0, 1, 2, 3])
@pytest.mark.parametrize("count", [1, 2, 255, 256])
def test_gather_counts_and_alignments(gpu, count, align):
    _, cur, res = _case(gpu, count, None, align)
    assert res == (count, sum(_lens(count))) and cur.stopped == 0


@pytest.mark.parametrize("count", [2, 255, 256])
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_gather_stops_in_front_of_a_failing_status(gpu, count, where):
    bad = {"first": 0, "middle": count // 2, "last": count - 1}[where]
    _, cur, res = _case(gpu, count, bad, 1)
    assert res[0] == bad and cur.stopped == 1


def test_gather_single_record_of_every_short_length(gpu):
    for n in (0, 1, 2, 3, 4, 5, 7, 8, 9):
        for align in range(4):
            _case(gpu, 1, None, align, lens=[n])
    _case(gpu, 1, 0, 0, lens=[5])
    _case(gpu, 1, None, 3, lens=[FULL])


def test_gather_other_stops(gpu):
    # content above 2^14 stops like a status; so do statuses 2 and 5
    _, cur, res = _case(gpu, 4, None, 2, lens=[10, FULL + 1, 3, 3])
    assert res == (1, 10) and cur.stopped == 1
    for st in (2, 5):
        _, cur, res = _case(gpu, 4, None, 2, lens=[10, 6, 0, 3], status=[0, 0, st, 0])
        assert res == (2, 16) and cur.stopped == 1


def test_gather_incoming_stopped_cursor_delivers_nothing(gpu):
    for use_base in (False, True):
        img, cur, res = _case(gpu, 256, None, 1, cur=RR.Cursor(37, 1), use_base=use_base)
        assert res == (0, 0) and (cur.offset, cur.stopped) == (37, 1)


def test_gather_two_chained_chunks(gpu):
    """The second chunk lands where the first one's cursor ends, at any alignment that
    leaves it; a stop in the first silences the second."""
    for bad in (None, 200):
        lens1, lens2 = _lens(256), list(reversed(_lens(255)))
        status1 = [0] * 256
        if bad is not None:
            status1[bad] = 1
        src1 = fp.sentinel(256 * STRIDE, 0x17) ^ np.uint8(0xA5)
        src2 = fp.sentinel(255 * STRIDE, 0x29) ^ np.uint8(0x5A)
        dst = fp.sentinel(1024 + sum(lens1) + sum(lens2), 0x3C)
        w1 = RR.gather_model(src1, STRIDE, status1, lens1, dst, 259, RR.Cursor(), True)
        g1 = _gather(gpu, src1, status1, lens1, dst, 259, RR.Cursor(), True)
        RR.gather_check(g1[0], g1[1], g1[2], *w1)
        c1 = RR.Cursor(*g1[1])
        w2 = RR.gather_model(src2, STRIDE, [0] * 255, lens2, w1[0], 259, c1, True)
        g2 = _gather(gpu, src2, [0] * 255, lens2, g1[0], 259, c1, True)
        RR.gather_check(g2[0], g2[1], g2[2], *w2)
        assert (g2[2][0] == 255) == (bad is None)
