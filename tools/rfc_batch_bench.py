#!/usr/bin/env python3
"""Rate of the RFC 8439 record batch (sg_seal_batch_rfc8439 / sg_open_batch_rfc8439)
beside the draft calls on the same records.  Prints one JSON line.

Two batches, both device-resident TLS records:

* ``uniform``: ``--records`` (default 2^18) records of 16 KiB, one key, sequential
  seq -- the wave-per-record kernel in both constructions;
* ``mixed``: ``--mixed-records`` records of the C2 Zipf layout (64 B-16 KiB, 256
  connection keys, suruga_amd.workloads.c2_layout) -- both constructions run it on
  the packed kernel, the buckets and the size classes.  A third leg,
  ``rfc_classes``, runs the RFC batch with ``sg_set_packed(0)`` and
  ``sg_set_lockstep(0)``: the size classes alone, the only route the RFC batch had
  before the routed kernels existed in its form; ``routed_vs_classes_*`` is the
  routed RFC time over that leg's.  ``routes`` holds every leg's route populations
  (``sg_last_batch_routes``), and the two RFC legs' sealed images must be equal.

The legs alternate launch by launch in one process (every seal and every open once
per round), so they share the clock the board holds; every round runs them in another
order (a seeded shuffle, tools/ab_legs.py), so that no leg always follows the same one.
Each leg reports the median of ``--reps`` launches after ``--warmup`` from HIP
events, GiB/s of payload, and ``spread`` = (max - min) / median.
``rfc_vs_draft_*`` is RFC time over draft time.  ``timing`` splits each
construction's launches into keying pre-pass and record kernel
(sg_timing_read), from a separate short pass.  A sample of sealed records of each
batch is compared with tests/rfc8439_ref.py, every byte and the tag.

    python tools/rfc_batch_bench.py [--records 262144] [--mixed-records 262144] [--reps 25]

``--records 0`` skips the uniform batch.  ``clock`` (uniform) and ``mixed.clock`` are
the shader clock and board power sampled while each batch's legs ran.
"""
from __future__ import annotations

import argparse
import json
import struct
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ab_legs  # noqa: E402  (tools/, this script's directory)

REC = 16384
SEED = 0x7266635F
SAMPLE = 24


def tls_nonce(iv: bytes, seq: int) -> bytes:
    return bytes(a ^ b for a, b in zip(iv, bytes(4) + struct.pack(">Q", seq)))


def make_uniform(count: int):
    import torch

    from suruga_amd import batch as B

    key = bytes(range(32))
    iv = bytes(range(0x80, 0x8C))
    keys = torch.tensor(list(key), dtype=torch.uint8, device="cuda").view(1, 32)
    ivs = torch.tensor(list(iv), dtype=torch.uint8, device="cuda").view(1, 12)
    pt = torch.empty(count * REC, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, REC, REC, count, SEED)
    cs = REC + 128  # 128-byte aligned slots, as bench.py's C1
    back = torch.empty(count * REC, dtype=torch.uint8, device="cuda")
    ws = torch.empty(B.workspace_size(count), dtype=torch.uint8, device="cuda")
    legs, cts, sts = {}, {}, {}
    for name, extra in (("draft", {}), ("rfc", dict(rfc8439=True, ivs=ivs))):
        ct = torch.empty(count * cs, dtype=torch.uint8, device="cuda")
        st = torch.zeros(count, dtype=torch.uint8, device="cuda")
        legs[name] = (B.Batch(count=count, keys=keys, inp=pt, out=ct, uniform_len=REC, in_stride=REC, out_stride=cs,
                              seq0=7, workspace=ws, **extra),
                      B.Batch(count=count, keys=keys, inp=ct, out=back, uniform_len=REC + 16, in_stride=cs,
                              out_stride=REC, seq0=7, status=st, workspace=ws, **extra))
        cts[name], sts[name] = ct, st

    def record(i):  # (key, nonce, ad, pt, sealed) of record i of the RFC leg
        seq = 7 + i
        ad = struct.pack(">QBBBH", seq, 23, 3, 3, REC)
        return (key, tls_nonce(iv, seq), ad, pt[i * REC:(i + 1) * REC].cpu().numpy().tobytes(),
                cts["rfc"][i * cs:i * cs + REC + 16].cpu().numpy().tobytes())

    return dict(count=count, payload=count * REC, legs=legs, pt=pt, back=back, sts=sts, record=record,
                desc=f"{count} x {REC} B TLS records, one key")


def make_mixed(count: int):
    import numpy as np
    import torch

    from suruga_amd import batch as B
    from suruga_amd import workloads as W

    lay = W.c2_layout(count)
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")  # noqa: E731
    keys_h = bytes(lay.keys)
    num_keys = len(keys_h) // 32
    ivs_h = np.random.default_rng(7905).integers(0, 256, 12 * num_keys, dtype=np.uint8).tobytes()
    keys = torch.tensor(list(keys_h), dtype=torch.uint8, device="cuda").view(-1, 32)
    ivs = torch.tensor(list(ivs_h), dtype=torch.uint8, device="cuda").view(-1, 12)
    pt = torch.empty(lay.pt_bytes, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, 0, lay.pt_bytes, 1, SEED)
    back = torch.empty(lay.pt_bytes, dtype=torch.uint8, device="cuda")
    ws = torch.empty(B.workspace_size(count), dtype=torch.uint8, device="cuda")
    lens, olens = t32(lay.lens), t32(lay.lens + 16)
    in_off, out_off, kidx, seqs = t64(lay.in_off), t64(lay.out_off), t32(lay.key_index), t64(lay.seq)
    maxl = int(lay.lens.max())
    legs, cts, sts = {}, {}, {}
    for name, extra in (("draft", {}), ("rfc", dict(rfc8439=True, ivs=ivs)),
                        ("rfc_classes", dict(rfc8439=True, ivs=ivs))):
        ct = torch.empty(lay.ct_bytes, dtype=torch.uint8, device="cuda")
        st = torch.zeros(count, dtype=torch.uint8, device="cuda")
        legs[name] = (B.Batch(count=count, keys=keys, inp=pt, out=ct, lens=lens, max_len=maxl, in_off=in_off,
                              out_off=out_off, key_index=kidx, seq=seqs, workspace=ws, **extra),
                      B.Batch(count=count, keys=keys, inp=ct, out=back, lens=olens, max_len=maxl + 16, in_off=out_off,
                              out_off=in_off, key_index=kidx, seq=seqs, status=st, workspace=ws, **extra))
        cts[name], sts[name] = ct, st

    def record(i):
        n, k, seq = int(lay.lens[i]), int(lay.key_index[i]), int(lay.seq[i])
        io, oo = int(lay.in_off[i]), int(lay.out_off[i])
        ad = struct.pack(">QBBBH", seq, 23, 3, 3, n)
        return (keys_h[32 * k:32 * k + 32], tls_nonce(ivs_h[12 * k:12 * k + 12], seq), ad,
                pt[io:io + n].cpu().numpy().tobytes(), cts["rfc"][oo:oo + n + 16].cpu().numpy().tobytes())

    return dict(count=count, payload=int(lay.payload), legs=legs, pt=pt, back=back, sts=sts, record=record,
                forms={"rfc_classes": dict(lockstep=0, packed=0)}, same=[(cts["rfc"], cts["rfc_classes"])],
                desc=f"{count} Zipf(1.1) TLS records 64 B-16 KiB (mean {lay.payload / count:.0f} B), {num_keys} keys")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import batch as B

    from gpu_support import kernel_forms  # sets the switches and puts them back after the launch

    from suruga_amd import _native

    lib = _native.load()
    names = list(w["legs"])
    forms = w.get("forms", {})
    routes = {}

    def leg(name, d):
        def fn():
            with kernel_forms(lib, **forms.get(name, {})):
                (B.open_ if d else B.seal)(w["legs"][name][d])
            routes.setdefault(f"{name}_{'open' if d else 'seal'}", B.last_routes())
        return f"{name}_{'open' if d else 'seal'}", fn

    times = ab_legs.timed_legs(dict(leg(name, d) for d in (0, 1) for name in names), reps, warmup)
    for name in names:
        assert int(w["sts"][name].sum().item()) == 0, f"{name}: open status"
    assert torch.equal(w["back"], w["pt"]), "round trip"
    for a, b in w.get("same", []):
        assert torch.equal(a, b), "the routed and the class-only RFC images differ"
    out = {"batch": w["desc"], "payload_bytes": w["payload"]}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["payload"])
    for d in ("seal", "open"):
        out[f"rfc_vs_draft_{d}"] = round(out[f"rfc_{d}"]["ms"] / out[f"draft_{d}"]["ms"], 4)
        if "rfc_classes" in names:
            out[f"routed_vs_classes_{d}"] = round(out[f"rfc_{d}"]["ms"] / out[f"rfc_classes_{d}"]["ms"], 4)
    out["routes"] = routes
    # where the time goes: keying pre-pass and record kernel of each construction
    out["timing"] = {}
    for name in ("draft", "rfc"):
        B.set_timing(True)
        for _ in range(5):
            B.seal(w["legs"][name][0])
            B.open_(w["legs"][name][1])
        torch.cuda.synchronize()
        t = B.timing_read()
        B.set_timing(False)
        out["timing"][name] = {k: round(v, 5) for k, v in t.items() if k.endswith("_ms")}
    return out


def check(w: dict) -> dict:
    """A sample of the RFC leg's sealed records against tests/rfc8439_ref.py."""
    import rfc8439_ref as R

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        key, nonce, ad, pt, sealed = w["record"](i)
        assert sealed == R.seal(key, nonce, pt, ad), f"record {i} differs from the RFC 8439 reference"
    ossl = R.openssl()
    if ossl is not None:
        key, nonce, ad, pt, sealed = w["record"](idx[-1])
        assert sealed == ossl.seal(key, nonce, pt, ad), "record differs from OpenSSL"
    return {"records_checked": len(idx), "openssl": ossl.version if ossl else None,
            "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 18, help="uniform 16 KiB batch (0: skip)")
    ap.add_argument("--mixed-records", type=int, default=1 << 18, help="Zipf batch (0: skip)")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    import torch

    res, bus = ab_legs.prelude("rfc_batch_bench", args.reps, args.warmup)
    if args.records:
        w = make_uniform(args.records)
        with ab_legs.clock(bus) as res["clock"]:
            res["uniform"] = run(w, args.reps, args.warmup)
        res["uniform"]["check"] = check(w)
        del w
        torch.cuda.empty_cache()
    if args.mixed_records:
        w = make_mixed(args.mixed_records)
        with ab_legs.clock(bus) as clk:
            res["mixed"] = run(w, args.reps, args.warmup)
        res["mixed"]["clock"] = clk
        res["mixed"]["check"] = check(w)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
