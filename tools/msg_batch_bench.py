#!/usr/bin/env python3
"""Rate of the message batch (sg_seal_msg_batch / sg_open_msg_batch) next to the
single-message call on the same bytes.  Prints one JSON line.

Per shape (device-resident messages, 13 bytes of AD each, four keys, a nonce
per message), for seal and for open:

* ``a``: the batch call, all messages in one call.
* ``b``: the same items through sg_seal_msg_dev / sg_open_msg_dev one after the
  other on one stream -- what a caller could do before the batch call existed.
* ``c``: one message of the shape's total byte count through the single call:
  the tile loop's own ceiling.

Time from HIP events around each call (for ``b``: around the whole loop), median
of ``--reps`` launches after ``--warmup``; the legs alternate launch by launch in
one process, so they share the clock the board holds, which the sampler records
alongside; every round runs them in another order (a seeded shuffle,
tools/ab_legs.py), so that no leg always follows the same one.  ``spread`` of a leg is (max - min) / median over its repeats.
``a_beats_b``: (b - a) / b exceeds b's spread.

Checked inside the tool: the batch's output equals the loop's byte for byte,
both directions, and a seeded sample of messages equals the CPU oracle.

Shapes: 16,384 x 64 KiB, 1,024 x 1 MiB, 64 x 16 MiB, and a seeded log-uniform
mix of 32 KiB .. 16 MiB totalling about 1 GiB.

    python tools/msg_batch_bench.py [--shapes 64k,1m,16m,mix] [--reps 25] [--groups 0]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ab_legs  # noqa: E402  (tools/, this script's directory)

ADLEN = 13
NUM_KEYS = 4
SAMPLE = 4
SHAPES = {"64k": (16384, 64 << 10), "1m": (1024, 1 << 20), "16m": (64, 16 << 20)}


def lengths_of(shape: str):
    if shape in SHAPES:
        count, n = SHAPES[shape]
        return [n] * count
    assert shape == "mix"
    rng = np.random.default_rng(0x6D6978)
    out, total = [], 0
    while total < (1 << 30):
        n = int(np.exp(rng.uniform(np.log(32 << 10), np.log(16 << 20)))) & ~15  # contiguous 16-byte aligned messages
        out.append(n)
        total += n
    return out


def run_shape(shape: str, reps: int, warmup: int, bus: str) -> dict:
    import torch

    from oracle_ffi import oracle
    from suruga_amd import _native as N
    from suruga_amd import msg

    lib = N.load()
    lens = lengths_of(shape)
    count, total = len(lens), sum(lens)
    in_off = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    out_off = np.concatenate([[0], np.cumsum([n + 16 for n in lens])[:-1]]).astype(np.int64)
    rng = np.random.default_rng(count)
    keys_h = rng.bytes(32 * NUM_KEYS)
    nonces = [i.to_bytes(4, "little") + rng.bytes(4) for i in range(count)]
    ads_h = rng.bytes(16 * count)  # message i's AD: 13 bytes at 16 i

    def dev(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    keys, ads = dev(keys_h).view(NUM_KEYS, 32), dev(ads_h)
    pt = torch.randint(0, 256, (total,), dtype=torch.uint8, device="cuda")
    ct = {leg: torch.empty(total + 16 * count, dtype=torch.uint8, device="cuda") for leg in "ab"}
    back = {leg: torch.empty(total, dtype=torch.uint8, device="cuda") for leg in "ab"}
    ct["c"] = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
    back["c"] = torch.empty(total, dtype=torch.uint8, device="cuda")
    st = {"a": torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda"),
          "b": torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda"),
          "c": torch.full((1,), 0xFF, dtype=torch.uint8, device="cuda")}
    ws_one = torch.empty(msg.workspace_size(), dtype=torch.uint8, device="cuda")
    ws_batch = torch.empty(msg.batch_workspace_size(count), dtype=torch.uint8, device="cuda")
    # a stream of its own: with a non-NULL stream the calls are asynchronous, so the loop of leg b
    # enqueues back to back instead of waiting for every message (NULL = synchronous)
    stream = torch.cuda.Stream()
    sh = int(stream.cuda_stream)
    assert sh != 0
    torch.cuda.synchronize()

    # ---- the calls, built once: the timed region is the library call alone
    def items_of(src, src_off, extra, dst, dst_off):
        arr = (N.SgMsgItem * count)()
        for i in range(count):
            it = arr[i]
            it.key_index = i % NUM_KEYS
            it.nonce[:] = nonces[i]
            it.ad, it.ad_len = ads.data_ptr() + 16 * i, ADLEN
            it.in_, it.in_len = src.data_ptr() + int(src_off[i]), lens[i] + extra
            it.out = dst.data_ptr() + int(dst_off[i])
        return arr

    def batch_of(arr, status):
        b = N.SgMsgBatch()
        b.count, b.flags, b.keys, b.num_keys, b.items = count, 0, keys.data_ptr(), NUM_KEYS, arr
        b.status = status.data_ptr() if status is not None else None
        b.stream, b.workspace, b.workspace_size = sh, ws_batch.data_ptr(), ws_batch.numel()
        return b

    def singles_of(arr, status):
        out = (N.SgMsg * count)()
        for i in range(count):
            m, it = out[i], arr[i]
            m.key = keys.data_ptr() + 32 * it.key_index
            m.nonce[:] = nonces[i]
            m.ad, m.ad_len, m.in_, m.in_len, m.out = it.ad, it.ad_len, it.in_, it.in_len, it.out
            m.status = status.data_ptr() + i if status is not None else None
            m.stream, m.workspace, m.workspace_size = sh, ws_one.data_ptr(), ws_one.numel()
        return out

    def one(src, n_in, dst, status):
        m = N.SgMsg()
        m.key = keys.data_ptr()
        m.nonce[:] = nonces[0]
        m.ad, m.ad_len, m.in_, m.in_len, m.out = ads.data_ptr(), ADLEN, src.data_ptr(), n_in, dst.data_ptr()
        m.status = status.data_ptr() if status is not None else None
        m.stream, m.workspace, m.workspace_size = sh, ws_one.data_ptr(), ws_one.numel()
        return m

    seal_items = {leg: items_of(pt, in_off, 0, ct[leg], out_off) for leg in "ab"}
    open_items = {leg: items_of(ct[leg], out_off, 16, back[leg], in_off) for leg in "ab"}
    a_seal, a_open = batch_of(seal_items["a"], None), batch_of(open_items["a"], st["a"])
    b_seal, b_open = singles_of(seal_items["b"], None), singles_of(open_items["b"], st["b"])
    c_seal, c_open = one(pt, total, ct["c"], None), one(ct["c"], total + 16, back["c"], st["c"])

    def loop(fn, arr):
        def go():
            for i in range(count):
                rc = fn(C.byref(arr[i]))
                assert rc == 0, (rc, N.last_error())
        return go

    def call(fn, arg):
        def go():
            rc = fn(C.byref(arg))
            assert rc == 0, (rc, N.last_error())
        return go

    legs = {
        "a_seal": call(lib.sg_seal_msg_batch, a_seal), "b_seal": loop(lib.sg_seal_msg_dev, b_seal),
        "c_seal": call(lib.sg_seal_msg_dev, c_seal),
        "a_open": call(lib.sg_open_msg_batch, a_open), "b_open": loop(lib.sg_open_msg_dev, b_open),
        "c_open": call(lib.sg_open_msg_dev, c_open),
    }
    # the clock the board holds while the legs are timed; the checks run apart from it
    with ab_legs.clock(bus) as clk:
        times = ab_legs.timed_legs(legs, reps, warmup, stream)

    # ---- checks: statuses, round trips, a == b byte for byte, a sample against the oracle
    assert all(int(s.sum().item()) == 0 for s in st.values()), "open status"
    assert all(torch.equal(back[leg], pt) for leg in "abc"), "round trip"
    assert torch.equal(ct["a"], ct["b"]), "the batch's ciphertext and tags differ from the loop's"
    orc = oracle()
    sample = ab_legs.sample_indices(count, SAMPLE)
    t0 = time.perf_counter()
    for i in sample:
        got = ct["a"][int(out_off[i]):int(out_off[i]) + lens[i] + 16].cpu().numpy().tobytes()
        want = orc.seal(keys_h[32 * (i % NUM_KEYS):32 * (i % NUM_KEYS) + 32], nonces[i],
                        pt[int(in_off[i]):int(in_off[i]) + lens[i]].cpu().numpy().tobytes(), ads_h[16 * i:16 * i + ADLEN])
        assert got == want, f"message {i} differs from the oracle"
    plan = msg.batch_plan_for(lens, [ADLEN] * count, max(msg.set_groups(-1), 0))
    out = {"shape": shape, "count": count, "bytes": total, "adlen": ADLEN, "min_len": min(lens), "max_len": max(lens),
           "plan": {k: plan[k] for k in ("tiles", "tiles_per_group", "groups", "segments")},
           "a_equals_b": True, "oracle_sample": sample, "oracle_s": round(time.perf_counter() - t0, 2),
           "clock": clk}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, total)
    for d in ("seal", "open"):
        a, b, c = out[f"a_{d}"], out[f"b_{d}"], out[f"c_{d}"]
        out[f"a_vs_b_{d}"] = round(a["ms"] / b["ms"], 4)
        out[f"a_vs_c_{d}"] = round(a["ms"] / c["ms"], 4)
        out[f"a_beats_b_{d}"] = (b["ms"] - a["ms"]) / b["ms"] > b["spread"]
        out[f"a_within_c_spread_{d}"] = (a["ms"] - c["ms"]) / c["ms"] <= c["spread"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--shapes", default="64k,1m,16m,mix")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=None, help="sg_set_msg_groups (default: leave the setting)")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    import torch

    from suruga_amd import msg

    res, bus = ab_legs.prelude("msg_batch_bench", args.reps, args.warmup)
    if args.groups is not None:
        msg.set_groups(args.groups)
    res.update(msg_groups=msg.set_groups(-1), shapes=[])
    for shape in args.shapes.split(","):
        res["shapes"].append(run_shape(shape, args.reps, args.warmup, bus))
        torch.cuda.empty_cache()
    res["a_beats_b_everywhere"] = all(r[f"a_beats_b_{d}"] for r in res["shapes"] for d in ("seal", "open"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
