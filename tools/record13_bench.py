#!/usr/bin/env python3
"""The record layer over host memory in its three forms, in one process: the draft
(sg_write_records / sg_read_records), RFC 7905 (*_rfc7905) and TLS 1.3 (*_tls13),
each writing and reading the same application bytes as full 2^14-byte records from
and to pageable and registered host buffers; the TLS 1.3 read on pageable buffers
also with SG_RECORD13_GATHER on (the gather kernel packs the chunk into the pinned
staging; off, the default leg, the host copies record by record).

The method is tools/ab_legs.py's: every leg runs once per round, the rounds run the
legs in another (seeded) order each, and a leg's figure is the median over the
rounds with its spread (max - min) / median beside it.  A leg is timed wall-clock
around its calls, so every copy is inside the number; sg_record_timing's split is
that of the leg's fastest round, per GiB.  Shader clock and board power are sampled
(sysfs, read only) beside each leg.  Every leg's read-back is compared with the
input once, byte for byte.

What the numbers decide: the default of SG_RECORD13_GATHER --
the device form only if its median read time beats the host copy's by more than the
larger of the two legs' spreads -- and the TLS 1.3 / RFC 7905 time over the draft's
in the same process, which is written down with its spread and is no gate.

    python tools/record13_bench.py [--bytes 1073741824] [--call-bytes 67108864] [--rounds 5]
        [--json-out profiles/record13_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
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

KEY = bytes(range(32))
IV = bytes(range(100, 112))
FULL = 1 << 14
# (name, form, registered, SG_RECORD13_GATHER)
LEGS = [("draft", "draft", False, 0), ("draft+registered", "draft", True, 0),
        ("rfc7905", "rfc7905", False, 0), ("rfc7905+registered", "rfc7905", True, 0),
        ("tls13", "tls13", False, 0), ("tls13+registered", "tls13", True, 0),
        ("tls13+gather", "tls13", False, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bytes", type=int, default=1 << 30)
    ap.add_argument("--call-bytes", type=int, default=64 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--json-out")
    a = ap.parse_args()
    import numpy as np

    head, bus = ab_legs.prelude("record13_bench", a.rounds, 1)
    from suruga_amd import _native as N
    from suruga_amd import devmon

    lib = N.load()
    cpus, how = devmon.pin_to_gpu_node(bus)
    total = a.bytes // FULL * FULL
    data = {False: np.frombuffer(np.random.default_rng(0xC4).bytes(total), dtype=np.uint8).copy()}
    data[True] = data[False].copy()
    cap = lib.sg_wire_bound_tls13(total)
    wire = {r: np.zeros(cap, dtype=np.uint8) for r in (False, True)}
    back = {r: np.zeros(total, dtype=np.uint8) for r in (False, True)}
    for arr in (data[True], wire[True], back[True]):
        N.check(lib.sg_host_register(arr.ctypes.data, arr.nbytes))

    ctx = {}
    for form in ("draft", "rfc7905", "tls13"):
        for side in ("w", "r"):
            p = lib.sg_ctx_new(KEY, a.device)
            assert p, N.last_error()
            N.check(lib.sg_ctx_set_iv(p, IV))
            ctx[form, side] = p

    def split(acc):
        v = [C.c_double() for _ in range(4)]
        lib.sg_record_timing(*[C.byref(x) for x in v])
        for k, x in zip(("h2d", "kernel", "d2h", "host"), v):
            acc[k] = acc.get(k, 0.0) + x.value

    def write_all(form, reg, acc):
        wl = C.c_size_t(0)
        seq = pos = wpos = 0
        d, w = data[reg], wire[reg]
        while pos < total:
            n = min(a.call_bytes, total - pos)
            src, dst = C.c_void_p(d.ctypes.data + pos), C.c_void_p(w.ctypes.data + wpos)
            if form == "tls13":
                rc = lib.sg_write_records_tls13(ctx[form, "w"], seq, 23, src, n, dst, w.size - wpos, C.byref(wl))
            else:
                fn = lib.sg_write_records if form == "draft" else lib.sg_write_records_rfc7905
                rc = fn(ctx[form, "w"], seq, 23, 3, 3, src, n, dst, w.size - wpos, C.byref(wl))
            seq += N.check(rc)
            split(acc)
            pos += n
            wpos += wl.value
        return seq, wpos

    def read_all(form, reg, wlen, acc):
        res = N.SgReadResult()
        seq = pos = opos = 0
        w, o = wire[reg], back[reg]
        fn = {"draft": lib.sg_read_records, "rfc7905": lib.sg_read_records_rfc7905,
              "tls13": lib.sg_read_records_tls13}[form]
        pitch = 5 + FULL + (17 if form == "tls13" else 16)
        per_call = a.call_bytes // FULL * pitch
        while pos < wlen:
            n = min(per_call, wlen - pos)
            N.check(fn(ctx[form, "r"], seq, C.c_void_p(w.ctypes.data + pos), n, C.c_void_p(o.ctypes.data + opos),
                       o.size - opos, None, None, 1 << 20, C.byref(res)))
            if res.error != N.SG_OK:
                raise RuntimeError(f"{form}: record error {res.error} after {seq + res.records} records")
            split(acc)
            seq += res.records
            pos += res.consumed
            opos += res.out_len
        return seq, opos

    runs = {name: {"write": [], "read": [], "wsplit": [], "rsplit": [], "clk": []} for name, *_ in LEGS}
    correct = {}
    rnd = random.Random(0x13)
    for rd in range(a.rounds + 1):  # round 0 warms up (staging allocation, page faults) and checks
        order = LEGS[:]
        rnd.shuffle(order)
        for name, form, reg, gather in order:
            prev = lib.sg_set_record13_gather(gather)
            try:
                with ab_legs.clock(bus) as clk:
                    wacc, racc = {}, {}
                    t0 = time.perf_counter()
                    nrec, wlen = write_all(form, reg, wacc)
                    t1 = time.perf_counter()
                    if rd == 0:
                        back[reg][:] = 0
                        t1b = time.perf_counter()
                    else:
                        t1b = t1
                    rrec, olen = read_all(form, reg, wlen, racc)
                    t2 = time.perf_counter()
            finally:
                lib.sg_set_record13_gather(prev)
            if rd == 0:
                correct[name] = bool(rrec == nrec == total // FULL and olen == total and
                                     np.array_equal(back[reg], data[reg]))
                continue
            r = runs[name]
            r["write"].append((t1 - t0) * 1e3)
            r["read"].append((t2 - t1b) * 1e3)
            r["wsplit"].append(wacc)
            r["rsplit"].append(racc)
            r["clk"].append(clk)

    gib = total / 2**30

    def mean_of(clks, key):  # median over the rounds of the leg's mean while it ran
        v = [c[key]["mean"] for c in clks if c.get(key)]
        return round(statistics.median(v), 1) if v else None

    def leg(name):
        r = runs[name]
        per = lambda acc: {k + "_ms_per_gib": round(v / gib, 2) for k, v in acc.items()}  # noqa: E731
        fw, fr = r["write"].index(min(r["write"])), r["read"].index(min(r["read"]))
        return {"write": ab_legs.summary(r["write"], total), "read": ab_legs.summary(r["read"], total),
                "write_split": per(r["wsplit"][fw]), "read_split": per(r["rsplit"][fr]),
                "sclk_mhz": mean_of(r["clk"], "sclk_mhz"), "board_power_w": mean_of(r["clk"], "board_power_w"),
                "correct": correct[name]}

    legs = {name: leg(name) for name, *_ in LEGS}

    def over(x, y, side):  # leg x's median time over leg y's, and the larger spread of the two
        return {"ratio": round(legs[x][side]["ms"] / legs[y][side]["ms"], 4),
                "spread": max(legs[x][side]["spread"], legs[y][side]["spread"])}

    host, dev = legs["tls13"]["read"], legs["tls13+gather"]["read"]
    margin = max(host["spread"], dev["spread"])
    gain = (host["ms"] - dev["ms"]) / host["ms"]
    out = dict(head, bytes=total, call_bytes=a.call_bytes, records=total // FULL, pinned={"cpus": len(cpus) if cpus else None,
                                                                                         "how": how},
               note="wall clock around the calls, ms per leg-run of `bytes`; gib_s: content bytes at the median; "
                    "spread = (max - min) / median over the rounds; splits per GiB of the leg's fastest round",
               legs=legs,
               over_draft={f: {"write": over(f, "draft", "write"), "read": over(f, "draft", "read"),
                               "write_registered": over(f + "+registered", "draft+registered", "write"),
                               "read_registered": over(f + "+registered", "draft+registered", "read")}
                           for f in ("rfc7905", "tls13")},
               gather_switch={"host_copy_ms": host["ms"], "gather_ms": dev["ms"], "gain": round(gain, 4),
                              "larger_spread": margin, "default": 1 if gain > margin else 0,
                              "rule": "1 only if the gather leg's median read time is lower by more than the larger spread"},
               correct=all(correct.values()))
    print(json.dumps(out))
    if a.json_out:
        Path(a.json_out).write_text(json.dumps(out, indent=1) + "\n")
    for arr in (data[True], wire[True], back[True]):
        N.check(lib.sg_host_unregister(arr.ctypes.data))
    for p in ctx.values():
        lib.sg_ctx_free(p)
    sys.exit(0 if out["correct"] else 1)


if __name__ == "__main__":
    main()
