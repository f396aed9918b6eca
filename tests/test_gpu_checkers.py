"""The two device-side checkers, seen to fail and checked against the host.

sg_compare_records is the only round-trip judge of the full-size tests and of
bench.py's roundtrip_ok, whose buffers cannot go to the host; every call in the
tree expects 0 mismatches and gets 0.  Here single bits are flipped in one of
two equal device buffers and the count the kernel *adds* to *mismatches is
compared with numpy's count over host copies of the same bytes: in the 16-byte
vector loop and where its 256 threads wrap, in the byte tail, on the unaligned
path, in a stride gap (not part of any record), and in records past the
16384-block grid.

sg_fill_records is compared with oracle.fill_record byte for byte over a whole
sentinel buffer (tests/footprint.py): the 8-byte path and the byte path with its
tail guard, odd strides and bases, the stride = 0, count = 1 form of the bench's
mixed workload, record numbers at and above 2^32, where (j0 + j) << 32 wraps,
and seeds with the top bit set.  Gaps and the 256-byte margins stay sentinel.

footprint.run_whole, the runner of every whole-buffer test, is given calls that
write through the device tensors it hands out: the right bytes pass, and a byte
behind the record, a changed input byte and a touched status tail each fail
(every way its check can fail: tests/test_gpu_support_model.py, on the CPU).
"""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import footprint as fp
from gpu_support import dev_u8 as to_dev

pytestmark = pytest.mark.gpu

M = fp.MARGIN
BASES = (0, 1, 4, 8, 15)
COMPARE_LENGTHS = (1, 15, 16, 17, 31, 32, 33, 255, 4097, 16384)
WRAP = range(4079, 4113)  # thread 255 of the vector loop's first pass ends at byte 4095, thread 0 goes on at 4096


def strides_of(n: int):
    return sorted({n, n + 1, fp.round_up(n, 16)})


def flip_positions(n: int):
    return sorted({p for p in (0, 15, 16, (n // 16) * 16, n - 1) if 0 <= p < n})


class Pair:
    """Two device buffers holding the same `count` records (at bases ba / bb, strides
    sa / sb, different bytes in the gaps) and host copies that see every flip."""

    def __init__(self, n, count, ba, bb, sa, sb, seed):
        rng = np.random.default_rng([n, count, ba, bb, sa, sb, seed])
        self.n, self.count, self.ba, self.bb, self.sa, self.sb = n, count, ba, bb, sa, sb
        recs = rng.integers(0, 256, (count, n), dtype=np.uint8)
        self.ha = rng.integers(0, 256, M + ba + count * sa + M, dtype=np.uint8)
        self.hb = rng.integers(0, 256, M + bb + count * sb + M, dtype=np.uint8)
        self.view(self.ha, ba, sa)[:] = recs
        self.view(self.hb, bb, sb)[:] = recs
        self.da, self.db = to_dev(self.ha), to_dev(self.hb)
        assert self.da.data_ptr() % 16 == 0 and self.db.data_ptr() % 16 == 0

    def view(self, h, base, stride):
        return np.lib.stride_tricks.as_strided(h[M + base:], (self.count, self.n), (stride, 1))

    def flip(self, which: int, rec: int, pos: int, bit: int = 0):
        """Flip one bit of byte pos of record rec (pos may lie in the stride gap) in buffer a (0) or b (1)."""
        h, d, base, stride = ((self.ha, self.da, self.ba, self.sa), (self.hb, self.db, self.bb, self.sb))[which]
        i = M + base + rec * stride + pos
        h[i] ^= 1 << bit
        d[i:i + 1].bitwise_xor_(1 << bit)

    def host_mismatches(self) -> int:
        """numpy's count of records that differ."""
        return int((self.view(self.ha, self.ba, self.sa) != self.view(self.hb, self.bb, self.sb)).any(axis=1).sum())

    def device_adds(self, initial: int) -> int:
        """What sg_compare_records adds to a counter that starts at `initial`."""
        import torch

        from suruga_amd import batch as B

        ctr = torch.full((3,), 0x7777, dtype=torch.int64, device="cuda")
        ctr[1] = initial
        B.compare_records(self.da[M + self.ba:], self.sa, self.db[M + self.bb:], self.sb, self.n, self.count, ctr[1:],
                          stream=0)
        got = ctr.cpu().tolist()
        assert got[0] == 0x7777 and got[2] == 0x7777, "the counter's neighbours changed"
        return got[1] - initial


_calls = itertools.count()


def check(pair: Pair, what):
    initial = 5 if next(_calls) & 1 else 0  # the call adds
    want = pair.host_mismatches()
    got = pair.device_adds(initial)
    assert got == want, (what, f"len={pair.n} count={pair.count} bases={pair.ba},{pair.bb} strides={pair.sa},{pair.sb}",
                         f"device adds {got}, numpy counts {want}")
    return want


@pytest.mark.parametrize("n", COMPARE_LENGTHS)
def test_compare_counts_each_flipped_record(gpu, n):
    """Every flip position alone (the vector loop's first bytes, the first tail byte, the
    last byte), bases of a and b independently, three strides, 1 and 3 records."""
    calls = 0
    for count in (1, 3):
        for ba in BASES:
            for bb in BASES:
                for s, stride in enumerate(strides_of(n)):
                    pair = Pair(n, count, ba, bb, stride, strides_of(n)[(s + ba + bb) % len(strides_of(n))], 1)
                    assert check(pair, "identical buffers") == 0
                    for j, pos in enumerate(flip_positions(n)):
                        rec, which = (j + ba) % count, (j + bb) & 1
                        pair.flip(which, rec, pos, j % 8)
                        assert check(pair, f"one flip, byte {pos} of record {rec}") == 1
                        pair.flip(which, rec, pos, j % 8)
                        calls += 1
                    # two flips in one record count once; with a third in another record, twice
                    pair.flip(0, count - 1, 0)
                    pair.flip(1, count - 1, n - 1, 7)
                    assert check(pair, "two flips in one record") == 1
                    if count > 1:
                        pair.flip(1, 0, n // 2, 3)
                        assert check(pair, "flips in two records") == 2
                    # a byte in the gap behind a record belongs to no record
                    for which, st in ((0, pair.sa), (1, pair.sb)):
                        if st > n:
                            before = pair.host_mismatches()
                            pair.flip(which, 0, n)
                            pair.flip(which, count - 1, st - 1, 5)
                            assert check(pair, "flips in the stride gap") == before
    assert calls >= 2 * 25 * 2 * len(flip_positions(n))


@pytest.mark.parametrize("aligned", [True, False])
def test_compare_sees_every_byte_where_the_vector_loop_wraps(gpu, aligned):
    """16 KiB records: bytes 4079..4112, around the place where thread 255's 16 bytes end
    and thread 0's second pass begins; on the byte path (odd base) the same positions."""
    n, count = 16384, 3
    for ba, bb in (((0, 0), (16, 0)) if aligned else ((1, 1), (0, 15), (4, 8), (15, 1))):
        pair = Pair(n, count, ba, bb, n if aligned else n + 1, fp.round_up(n, 16) + (0 if aligned else 1), 2)
        for pos in WRAP:
            rec = pos % count
            pair.flip(pos & 1, rec, pos, pos % 8)
            assert check(pair, f"one flip, byte {pos} of record {rec}") == 1
            pair.flip(pos & 1, rec, pos, pos % 8)
        assert check(pair, "identical buffers") == 0


@pytest.mark.parametrize("stride,ba,bb", [(16, 0, 0), (17, 0, 1), (16, 15, 0), (32, 4, 8)])
def test_compare_reaches_records_past_the_grid(gpu, stride, ba, bb):
    """16390 records on a grid of 16384 workgroups: records 16384.. are the second
    pass of workgroups 0..5."""
    n, count = 16, 16390
    pair = Pair(n, count, ba, bb, stride, stride, 3)
    assert check(pair, "identical buffers") == 0
    for k, rec in enumerate((0, 16383, 16384, 16389)):
        pair.flip(k & 1, rec, (5 * k) % n, k)
        assert check(pair, f"one flip in record {rec}") == 1
        pair.flip(k & 1, rec, (5 * k) % n, k)
    for k, rec in enumerate((0, 16383, 16384, 16389)):
        pair.flip(k & 1, rec, n - 1 - k, 7 - k)
        assert check(pair, f"flips in records up to {rec}") == k + 1
    if stride > n:
        pair.flip(0, 16389, n)
        assert check(pair, "a flip in the last record's stride gap") == 4


# ---------------------------------------------------------------------------
# sg_fill_records against oracle.fill_record
# ---------------------------------------------------------------------------
FILL_LENGTHS = (1, 7, 8, 9, 15, 16, 17, 1001, 16384)
FILL_BASES = (0, 1, 4, 7)
FILL_J0 = (0, 1, 2**32 - 1, 2**32, 2**40 + 3)
FILL_SEEDS = (0x8000000000000000, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15, 0x53555255)
FILL_COUNT = 5


def check_fill(oracle, n, stride, count, base, seed, j0):
    from suruga_amd import batch as B

    size = 2 * M + base + (count - 1) * stride + n
    parts = [(M + base + j * stride, oracle.fill_record(seed, j0 + j, n)) for j in range(count)]
    salt, tries = fp.pick_salt(size, parts, 0x0D)
    assert tries <= fp.MAX_SALT_TRIES
    d = to_dev(fp.sentinel(size, salt))
    assert d.data_ptr() % 8 == 0
    B.fill_records(d[M + base:], stride, n, count, seed, j0, stream=0)
    rs = [(o, o + n) for o, _ in parts]
    diff = fp.first_diff(d.cpu().numpy(), fp.image(size, salt, parts), rs)
    assert diff is None, f"len={n} stride={stride} count={count} base={base} seed={seed:#x} j0={j0:#x}: {diff}"


@pytest.mark.parametrize("n", FILL_LENGTHS)
def test_fill_matches_the_oracle_and_stays_inside_its_records(gpu, oracle, n):
    """The 8-byte path (len, stride and base all multiples of 8) and the byte path with
    its tail guard; whole-buffer equality, so gaps and margins stay sentinel."""
    k = 0
    for stride in (n, n + 1, n + 8):
        for base in FILL_BASES:
            for j0 in FILL_J0:
                check_fill(oracle, n, stride, FILL_COUNT, base, FILL_SEEDS[k % len(FILL_SEEDS)], j0)
                k += 1
    for seed in FILL_SEEDS:  # every seed on both paths
        check_fill(oracle, n, n + 8, FILL_COUNT, 0, seed, 7)
        check_fill(oracle, n, n + 1, FILL_COUNT, 1, seed, 7)


@pytest.mark.parametrize("base", FILL_BASES)
def test_fill_one_long_record_with_stride_zero(gpu, oracle, base):
    """The form bench.py's mixed workload uses: stride = 0, count = 1, one long odd length."""
    for k, j0 in enumerate(FILL_J0):
        check_fill(oracle, 100003, 0, 1, base, FILL_SEEDS[k % len(FILL_SEEDS)], j0)
    check_fill(oracle, 100000, 0, 1, base, FILL_SEEDS[0], 2**32)  # a multiple of 8: the 8-byte path at base 0


# ---------------------------------------------------------------------------
# footprint.run_whole: upload, call, download, check
# ---------------------------------------------------------------------------
def test_run_whole_hands_out_the_buffers_and_sees_what_a_call_did(gpu):
    import torch

    n, size = 40, 2 * M + 48
    rec = bytes(range(1, n + 1))
    want, rs = fp.image(size, 0x2B, [(M, rec)]), [(M, M + n)]

    def run(stray):
        def call(d):
            assert all(t.dtype == torch.uint8 and t.is_cuda and t.data_ptr() % 16 == 0 for t in d.values())
            d["out"][M:M + n] = torch.frombuffer(bytearray(rec), dtype=torch.uint8).cuda()
            d["status"][0] = 0
            if stray:
                d[stray[0]][stray[1]] ^= 1
            return "rc"

        return fp.run_whole(call, fp.sentinel(64, 0x2C), fp.sentinel(size, 0x2B), want, rs,
                            arrays={"status": fp.array_start(1, 0x51)})

    o = run(None)
    o.check([0], where=("right",))
    assert o.ret == "rc" and o.out[M:M + n].tobytes() == rec
    for stray, label in ((("out", M + n), "output"), (("out", M - 1), "output"), (("inp", 63), "input"),
                         (("status", 1), "status tail"), (("status", 0), "status")):
        with pytest.raises(AssertionError) as e:
            run(stray).check([0], where=(stray,))
        assert e.value.args[0][:2] == (stray, label)
