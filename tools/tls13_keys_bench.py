#!/usr/bin/env python3
"""TLS 1.3 traffic keys of a whole table: the device call (sg_tls13_traffic_keys_dev,
one launch over a secrets table in HBM) beside the host call (sg_tls13_traffic_keys,
16 threads, host memory) on the same 2^20 secrets, each without and with the KeyUpdate
ratchet -- four legs in one process.

The method is tools/ab_legs.py's, as tools/record13_bench.py applies it to host calls:
every leg runs once per round, the rounds run the legs in another (seeded) order each,
and a leg's figure is the median over the rounds with its spread (max - min) / median
beside it.  A leg is timed wall-clock around its call; the device legs run on the NULL
stream, where the call returns when the launch is done.  One such call is a fraction of a
millisecond, mostly the wait, and shorter than the clock sampler's period, so a device leg
then enqueues `--inner` more calls back to back on a stream between two HIP events:
event_ms is that time per launch, and the leg's clock is sampled over both parts.  The
host legs' output stays in host memory: the
copy of 44 bytes per row that a caller of the batch calls would add is not in their
number.  Shader clock and board power are sampled (sysfs, read only) beside each leg.
Round 0 warms up and checks: both forms' tables must be equal byte for byte.

Nothing is decided by the ratio: the device call's output is needed in HBM either way.
The tool writes down what was measured.

    python tools/tls13_keys_bench.py [--rows 1048576] [--rounds 7] [--threads 16]
        [--json-out profiles/tls13_keys_bench.json]
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
import ab_legs  # noqa: E402

LEGS = [("device", True, False), ("device+update", True, True), ("host", False, False), ("host+update", False, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--inner", type=int, default=32, help="launches between the two events of a device leg")
    ap.add_argument("--json-out")
    a = ap.parse_args()
    import ctypes as C

    import numpy as np
    import torch

    head, bus = ab_legs.prelude("tls13_keys_bench", a.rounds, 1)
    from suruga_amd import _native as N
    from suruga_amd import devmon
    from suruga_amd import keysched as K

    lib = N.load()
    cpus, how = devmon.pin_to_gpu_node(bus)
    rows = a.rows
    start = np.frombuffer(np.random.default_rng(0x13).bytes(32 * rows), dtype=np.uint8).reshape(rows, 32).copy()
    start[0], start[1] = 0, 0xFF
    # one secrets table per leg, so that a ratchet leg never moves another leg's input
    h_sec = {u: start.copy() for u in (False, True)}
    h_keys, h_ivs = np.empty((rows, 32), dtype=np.uint8), np.empty((rows, 12), dtype=np.uint8)
    d_sec = {u: torch.from_numpy(start.copy()).to("cuda") for u in (False, True)}
    d_keys = torch.empty((rows, 32), dtype=torch.uint8, device="cuda")
    d_ivs = torch.empty((rows, 12), dtype=torch.uint8, device="cuda")
    p = lambda x: x.ctypes.data_as(C.c_void_p)  # noqa: E731

    side = torch.cuda.Stream()

    def run(dev: bool, update: bool, stream=0):
        if dev:  # stream 0 is the NULL stream: the call waits
            K.tls13_traffic_keys_dev(d_sec[update], d_keys, d_ivs, update=update, stream=stream)
        else:
            N.check(lib.sg_tls13_traffic_keys(rows, p(h_sec[update]), p(h_keys), p(h_ivs), int(update), a.threads))

    # round 0: each form once per mode from the same secrets, tables compared whole
    correct = {}
    for update in (False, True):
        run(True, update)
        run(False, update)
        torch.cuda.synchronize()
        correct["update" if update else "plain"] = bool(
            np.array_equal(d_keys.cpu().numpy(), h_keys) and np.array_equal(d_ivs.cpu().numpy(), h_ivs)
            and np.array_equal(d_sec[update].cpu().numpy(), h_sec[update]))
    correct["ratcheted"] = bool(not np.array_equal(h_sec[True], start) and np.array_equal(h_sec[False], start))

    runs = {name: {"wall": [], "event": [], "clk": []} for name, *_ in LEGS}
    rnd = random.Random(0x13)
    for _ in range(a.rounds):
        order = LEGS[:]
        rnd.shuffle(order)
        for name, dev, update in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with ab_legs.clock(bus) as clk:
                t0 = time.perf_counter()
                run(dev, update)
                t1 = time.perf_counter()
                if dev:
                    e0.record(side)
                    for _ in range(a.inner):
                        run(dev, update, side)
                    e1.record(side)
                    e1.synchronize()
            r = runs[name]
            r["wall"].append((t1 - t0) * 1e3)
            if dev:
                r["event"].append(e0.elapsed_time(e1) / a.inner)
            r["clk"].append(clk)

    def mean_of(clks, key):
        v = [c[key]["mean"] for c in clks if c.get(key)]
        return round(statistics.median(v), 1) if v else None

    def leg(name, update):
        r = runs[name]
        out = ab_legs.summary(r["wall"], 32 * rows)
        del out["gib_s"]
        out["rows_per_us"] = round(rows / (out["ms"] * 1e3), 2)
        out["compressions_per_row"] = 10 if update else 6
        if r["event"]:
            ev = ab_legs.summary(r["event"], 32 * rows)
            out["event_ms"], out["event_spread"] = ev["ms"], ev["spread"]
        out["sclk_mhz"], out["board_power_w"] = mean_of(r["clk"], "sclk_mhz"), mean_of(r["clk"], "board_power_w")
        return out

    legs = {name: leg(name, update) for name, _, update in LEGS}
    ratio = {m: {"host_wall_over_device_wall": round(legs["host" + s]["ms"] / legs["device" + s]["ms"], 2),
                 "host_wall_over_device_launch": round(legs["host" + s]["ms"] / legs["device" + s]["event_ms"], 2),
                 "spread": max(legs["host" + s]["spread"], legs["device" + s]["spread"],
                               legs["device" + s]["event_spread"])}
             for m, s in (("plain", ""), ("update", "+update"))}
    d, du, h, hu = (legs[k] for k in ("device", "device+update", "host", "host+update"))
    row = (f"| TLS 1.3 traffic keys, {rows} rows | device: {d['event_ms']} ms per launch (spread {d['event_spread']}), "
           f"one waiting call {d['ms']} ms ({d['spread']}); with the ratchet {du['event_ms']} ms ({du['event_spread']}), "
           f"{du['ms']} ms ({du['spread']}); {d['sclk_mhz']} MHz | host, {a.threads} threads: {h['ms']} ms "
           f"({h['spread']}); with the ratchet {hu['ms']} ms ({hu['spread']}) |")
    out = dict(head, rows=rows, threads=a.threads, inner=a.inner,
               pinned={"cpus": len(cpus) if cpus else None, "how": how},
               note="ms: wall clock around one call over `rows` secrets (the device call on the NULL stream, which "
                    "waits); event_ms: per launch of `inner` device calls back to back on a stream between two HIP "
                    "events; spread = (max - min) / median over the rounds; the host legs leave their tables in "
                    "host memory",
               legs=legs, ratio=ratio, readme_row=row, correct=correct)
    print(json.dumps(out))
    print(row, file=sys.stderr)
    if a.json_out:
        Path(a.json_out).write_text(json.dumps(out, indent=1) + "\n")
    sys.exit(0 if all(correct.values()) else 1)


if __name__ == "__main__":
    main()
