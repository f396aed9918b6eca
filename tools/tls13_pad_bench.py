#!/usr/bin/env python3
"""Rate of the padded TLS 1.3 seal (sg_seal_batch_tls13_ex, pad_to = 64) and of the open of
its fragments on a mixed batch, routed to the packed kernel and on the size classes alone,
beside the RFC 7905 batch over the same lengths.  Prints one JSON line and writes it to
``--out`` (profiles/tls13_bucket_bench.json is the committed four-leg run;
profiles/tls13_pad_bench.json the three-leg run of before the bucket route).

One batch: ``--records`` (default 2^18) device-resident records, 256 connection keys.  The
inner lengths are tools/rfc_batch_bench.py's Zipf leg (suruga_amd.workloads.zipf_lengths:
64 B-16 KiB, multiples of 64); record i has inner_i - 1 - (i * 37 mod 64) content bytes, so
that pad_to = 64 pads it to inner_i and the content ends anywhere in the last block.  Four
legs:

* ``rfc7905``: sg_*_batch_rfc8439 in TLS mode over records of inner_i bytes, as routed
  (packed kernel, J = 2..4 buckets, size classes) -- the fastest comparable call there was
  before this one;
* ``tls13``: sg_seal_batch_tls13_ex with pad_to = 64 and sg_open_batch_tls13 of its
  fragments, as routed: inner lengths up to 4 KiB on the packed kernel in its TLS 1.3 form,
  the longer ones on the size classes (sg_set_tls13_buckets is off by default);
* ``tls13_classes``: the same calls under ``sg_set_packed(0)``: the size classes alone;
* ``tls13_buckets``: the calls of ``tls13`` under ``sg_set_tls13_buckets(1)``: inner lengths
  above 4 KiB on the J = 2..4 wave-per-record buckets in their TLS 1.3 form.

The legs alternate launch by launch in one process (the four seals and the four opens
once per round), every round in another order (a seeded shuffle, tools/ab_legs.py).  Each
leg reports the median of ``--reps`` launches after ``--warmup`` from HIP events, GiB/s of
inner plaintext, and ``spread`` = (max - min) / median; ``routes`` holds every leg's
``sg_last_batch_routes``.  ``packed_vs_classes_*`` and ``tls13_vs_rfc7905_*`` are time
ratios; ``packed_kept_*`` says, for seal and for open separately, whether the routed leg
beats the class-only leg by more than the larger of the two legs' spreads -- DESIGN.md
section 4.12's rule for keeping the packed route the default of the TLS 1.3 form.  The
second ratio is reported, not gated.  ``buckets_vs_tls13_*`` (the baseline: the default route
of the same call in the same process) and ``buckets_vs_rfc7905_*`` are the bucket leg's time
ratios, and ``buckets_recommended_*`` applies the same rule to the first: the switch is
recommended in a direction only if the bucket leg beats the default leg by more than the
larger of the two legs' spreads.  The three TLS 1.3 images must be equal, every open must
return type and content length, and a sample of fragments is compared with
tests/tls13_ref.py, every byte and the tag.

    python tools/tls13_pad_bench.py [--records 262144] [--reps 25] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import ab_legs  # noqa: E402  (tools/, this script's directory)

SEED = 0x746C7364
SAMPLE = 24
CTYPE = 23
PAD_TO = 64
NAMES = ("rfc7905", "tls13", "tls13_classes", "tls13_buckets")


def make(count: int):
    import numpy as np
    import torch

    from suruga_amd import batch as B
    from suruga_amd import workloads as W

    inner = W.zipf_lengths(count)  # multiples of 64 in 64..16384
    lens = (inner - 1 - (np.arange(count, dtype=np.uint32) * 37) % 64).astype(np.uint32)
    assert all(B.tls13_inner_len(int(lens[i]), PAD_TO) == int(inner[i]) for i in ab_legs.sample_indices(count, 256))
    slot_i = inner.astype(np.uint64)                           # content at the start of a 64-byte aligned slot
    slot_o = (inner.astype(np.uint64) + 16 + 15) // 16 * 16     # fragments back to back, 16-byte aligned
    in_off, out_off = np.zeros(count, dtype=np.uint64), np.zeros(count, dtype=np.uint64)
    in_off[1:], out_off[1:] = np.cumsum(slot_i[:-1]), np.cumsum(slot_o[:-1])
    pt_bytes, ct_bytes = int(slot_i.sum()), int(slot_o.sum())
    num_keys = 256
    idx = np.arange(count, dtype=np.uint64)
    kidx_h, seq_h = (idx % num_keys).astype(np.uint32), (idx // num_keys).astype(np.uint64)
    keys_h = b"".join(W.connection_key(j) for j in range(num_keys))
    ivs_h = np.random.default_rng(8446).integers(0, 256, 12 * num_keys, dtype=np.uint8).tobytes()

    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")  # noqa: E731
    keys = torch.tensor(list(keys_h), dtype=torch.uint8, device="cuda").view(-1, 32)
    ivs = torch.tensor(list(ivs_h), dtype=torch.uint8, device="cuda").view(-1, 12)
    pt = torch.empty(pt_bytes, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, 0, pt_bytes, 1, SEED)
    ws = torch.empty(B.workspace_size(count), dtype=torch.uint8, device="cuda")
    d_inner, d_lens, d_frag = t32(inner), t32(lens), t32(inner + 16)
    d_in, d_out, kidx, seqs = t64(in_off), t64(out_off), t32(kidx_h), t64(seq_h)
    common = dict(count=count, keys=keys, ivs=ivs, key_index=kidx, seq=seqs, workspace=ws, content_type=CTYPE)
    legs, cts, sts, backs, outs = {}, {}, {}, {}, {}
    for name in NAMES:
        t13 = name != "rfc7905"
        ct = torch.zeros(ct_bytes, dtype=torch.uint8, device="cuda")  # (zeros: the images are compared whole)
        back = torch.zeros(pt_bytes, dtype=torch.uint8, device="cuda")
        st = torch.zeros(count, dtype=torch.uint8, device="cuda")
        extra = dict(rfc8439=True)
        if t13:
            outs[name] = (torch.zeros(count, dtype=torch.uint8, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda"))
            extra = dict(inner_type=outs[name][0], content_len=outs[name][1])
        legs[name] = (B.Batch(inp=pt, out=ct, lens=d_lens if t13 else d_inner, max_len=int((lens if t13 else inner).max()),
                              in_off=d_in, out_off=d_out, **common, **extra),
                      B.Batch(inp=ct, out=back, lens=d_frag, max_len=int(inner.max()) + 16, in_off=d_out, out_off=d_in,
                              status=st, **common, **extra))
        cts[name], sts[name], backs[name] = ct, st, back

    def record(i):  # (key, iv, seq, content, fragment) of record i of the routed leg
        k, io, oo, n, m = int(kidx_h[i]), int(in_off[i]), int(out_off[i]), int(lens[i]), int(inner[i])
        return (keys_h[32 * k:32 * k + 32], ivs_h[12 * k:12 * k + 12], int(seq_h[i]), pt[io:io + n].cpu().numpy().tobytes(),
                cts["tls13"][oo:oo + m + 16].cpu().numpy().tobytes(), m - n - 1)

    return dict(count=count, payload=int(inner.astype(np.uint64).sum()), content=int(lens.astype(np.uint64).sum()), legs=legs,
                cts=cts, sts=sts, backs=backs, outs=outs, d_lens=d_lens, record=record,
                desc=f"{count} Zipf(1.1) inner lengths 64 B-16 KiB (mean {float(inner.mean()):.0f} B), content padded to 64, "
                     f"{num_keys} keys")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import _native
    from suruga_amd import batch as B

    from gpu_support import kernel_forms  # sets the switch and puts it back after the launch

    lib = _native.load()
    forms = {"tls13_classes": dict(packed=0), "tls13_buckets": dict(tls13_buckets=1)}
    routes = {}

    def leg(name, d):
        t13 = name != "rfc7905"

        def fn():
            with kernel_forms(lib, **forms.get(name, {})):
                if not t13:
                    (B.open_ if d else B.seal)(w["legs"][name][d])
                elif d:
                    B.open_tls13(w["legs"][name][d])
                else:
                    B.seal_tls13(w["legs"][name][d], pad_to=PAD_TO)
            routes.setdefault(f"{name}_{'open' if d else 'seal'}", B.last_routes())
        return f"{name}_{'open' if d else 'seal'}", fn

    times = ab_legs.timed_legs(dict(leg(name, d) for d in (0, 1) for name in NAMES), reps, warmup)
    for name in NAMES:
        assert int(w["sts"][name].sum().item()) == 0, f"{name}: open status"
        if name in w["outs"]:
            ty, cl = w["outs"][name]
            assert bool((ty == CTYPE).all()) and torch.equal(cl, w["d_lens"]), f"{name}: inner type / content length"
    assert torch.equal(w["cts"]["tls13"], w["cts"]["tls13_classes"]), "the routed and the class-only images differ"
    assert torch.equal(w["backs"]["tls13"], w["backs"]["tls13_classes"]), "the routed and the class-only opens differ"
    assert torch.equal(w["cts"]["tls13_buckets"], w["cts"]["tls13"]), "the bucket leg's and the default route's images differ"
    assert torch.equal(w["backs"]["tls13_buckets"], w["backs"]["tls13"]), "the bucket leg's and the default route's opens differ"
    out = {"batch": w["desc"], "payload_bytes": w["payload"], "content_bytes": w["content"], "pad_to": PAD_TO}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["payload"])
    for d in ("seal", "open"):
        out[f"packed_vs_classes_{d}"] = round(out[f"tls13_{d}"]["ms"] / out[f"tls13_classes_{d}"]["ms"], 4)
        out[f"tls13_vs_rfc7905_{d}"] = round(out[f"tls13_{d}"]["ms"] / out[f"rfc7905_{d}"]["ms"], 4)
        spread = max(out[f"tls13_{d}"]["spread"], out[f"tls13_classes_{d}"]["spread"])
        out[f"packed_kept_{d}"] = out[f"packed_vs_classes_{d}"] < 1.0 - spread
        out[f"buckets_vs_tls13_{d}"] = round(out[f"tls13_buckets_{d}"]["ms"] / out[f"tls13_{d}"]["ms"], 4)
        out[f"buckets_vs_rfc7905_{d}"] = round(out[f"tls13_buckets_{d}"]["ms"] / out[f"rfc7905_{d}"]["ms"], 4)
        spread = max(out[f"tls13_buckets_{d}"]["spread"], out[f"tls13_{d}"]["spread"])
        out[f"buckets_recommended_{d}"] = out[f"buckets_vs_tls13_{d}"] < 1.0 - spread
    out["routes"] = routes
    return out


def check(w: dict) -> dict:
    """A sample of the routed leg's fragments against tests/tls13_ref.py."""
    import tls13_ref as T

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        key, iv, seq, content, frag, pad = w["record"](i)
        assert frag == T.seal(key, iv, seq, content, CTYPE, pad), f"record {i} differs from the TLS 1.3 reference"
    return {"records_checked": len(idx), "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=ROOT / "profiles" / "tls13_bucket_bench.json", help="where the JSON is written")
    args = ap.parse_args()

    res, bus = ab_legs.prelude("tls13_pad_bench", args.reps, args.warmup)
    w = make(args.records)
    with ab_legs.clock(bus) as res["clock"]:
        res["mixed"] = run(w, args.reps, args.warmup)
    res["mixed"]["check"] = check(w)
    line = json.dumps(res)
    args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
