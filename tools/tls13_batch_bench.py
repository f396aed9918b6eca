#!/usr/bin/env python3
"""Rate of the TLS 1.3 record batch (sg_seal_batch_tls13 / sg_open_batch_tls13) on full
records beside the RFC 7905 batch on the same content.  Prints one JSON line and, with
``--out``, writes it to a file (profiles/tls13_batch_bench.json is the committed run).

One batch: ``--records`` (default 2^18) device-resident records of 2^14 content bytes,
one key, sequential sequence numbers.  Three legs:

* ``rfc7905``: sg_*_batch_rfc8439 in TLS mode, the uniform 16 KiB batch on the
  wave-per-record kernel -- the fastest comparable call there was before this one;
* ``tls13``: sg_*_batch_tls13 as routed: the wave-per-record kernel, the keying pre-pass
  taking the inner type byte (``sg_batch_tls13_route`` must say 1);
* ``tls13_classes``: the same call under ``sg_set_lockstep(0)``: size class 7, which is
  also what a TLS 1.3 caller got from the RFC batch in explicit mode (route 0).

The legs alternate launch by launch in one process (the three seals and the three
opens once per round), so they share the clock the board holds; every round runs them
in another order (a seeded shuffle, tools/ab_legs.py), so that no leg always follows
the same one (the board is power-managed: a launch behind the slow class-only leg finds
a higher clock than one behind a wave-per-record leg).  Each leg reports the
median of ``--reps`` launches after ``--warmup`` from HIP events, GiB/s of content, and
``spread`` = (max - min) / median.  ``routed_vs_classes_*`` and ``routed_vs_rfc7905_*``
are time ratios; ``route_kept`` says whether the routed leg beats the class-only leg by
more than the larger of the two legs' spreads, seal and open.  ``timing`` splits the
launches into keying pre-pass and record kernel (sg_timing_read), from a separate short
pass.  The two TLS 1.3 images must be equal, every open must return the content, type and
length, and a sample of sealed records is compared with tests/tls13_ref.py, every byte
and the tag (one of them with OpenSSL where libcrypto loads).

    python tools/tls13_batch_bench.py [--records 262144] [--reps 48] [--out FILE]

``clock`` is the shader clock and board power sampled while the legs ran.
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

REC = 16384
SEED = 0x746C7313
SAMPLE = 24
CTYPE = 23
SEQ0 = 7


def make(count: int):
    import torch

    from suruga_amd import batch as B

    key = bytes(range(32))
    iv = bytes(range(0x80, 0x8C))
    keys = torch.tensor(list(key), dtype=torch.uint8, device="cuda").view(1, 32)
    ivs = torch.tensor(list(iv), dtype=torch.uint8, device="cuda").view(1, 12)
    pt = torch.empty(count * REC, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, REC, REC, count, SEED)
    cs = REC + 128  # 128-byte aligned slots, as bench.py's C1; holds the 2^14 + 17 byte fragment too
    ws = torch.empty(B.workspace_size(count), dtype=torch.uint8, device="cuda")
    legs, cts, sts, backs, outs = {}, {}, {}, {}, {}
    for name in ("rfc7905", "tls13", "tls13_classes"):
        t13 = name != "rfc7905"
        ct = torch.empty(count * cs, dtype=torch.uint8, device="cuda")
        st = torch.zeros(count, dtype=torch.uint8, device="cuda")
        bs = REC + 128 if t13 else REC  # the inner plaintext is one byte longer: 128-byte aligned slots again
        back = torch.empty(count * bs, dtype=torch.uint8, device="cuda")
        common = dict(count=count, keys=keys, ivs=ivs, seq0=SEQ0, workspace=ws, content_type=CTYPE)
        extra = {}
        if t13:
            outs[name] = (torch.zeros(count, dtype=torch.uint8, device="cuda"), torch.zeros(count, dtype=torch.int32, device="cuda"))
            extra = dict(inner_type=outs[name][0], content_len=outs[name][1])
        else:
            common["rfc8439"] = True
        legs[name] = (B.Batch(inp=pt, out=ct, uniform_len=REC, in_stride=REC, out_stride=cs, **common),
                      B.Batch(inp=ct, out=back, uniform_len=REC + (17 if t13 else 16), in_stride=cs, out_stride=bs, status=st,
                              **common, **extra))
        cts[name], sts[name], backs[name] = ct, st, (back, bs)

    def record(i):  # (key, iv, seq, content, fragment) of record i of the routed leg
        return (key, iv, SEQ0 + i, pt[i * REC:(i + 1) * REC].cpu().numpy().tobytes(),
                cts["tls13"][i * cs:i * cs + REC + 17].cpu().numpy().tobytes())

    return dict(count=count, payload=count * REC, legs=legs, pt=pt, cts=cts, sts=sts, backs=backs, outs=outs, record=record,
                desc=f"{count} x {REC} B of content, one key")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import _native
    from suruga_amd import batch as B

    from gpu_support import kernel_forms  # sets the switch and puts it back after the launch

    lib = _native.load()
    names = list(w["legs"])
    forms = {"tls13_classes": dict(lockstep=0)}
    routes = {}

    def leg(name, d):
        t13 = name != "rfc7905"
        call = (B.open_tls13 if d else B.seal_tls13) if t13 else (B.open_ if d else B.seal)

        def fn():
            with kernel_forms(lib, **forms.get(name, {})):
                if t13:
                    routes.setdefault(f"{name}_{'open' if d else 'seal'}", B.tls13_route(w["legs"][name][d], bool(d)))
                call(w["legs"][name][d])
        return f"{name}_{'open' if d else 'seal'}", fn

    times = ab_legs.timed_legs(dict(leg(name, d) for d in (0, 1) for name in names), reps, warmup)
    count = w["count"]
    for name in names:
        assert int(w["sts"][name].sum().item()) == 0, f"{name}: open status"
        back, bs = w["backs"][name]
        assert torch.equal(back.view(count, bs)[:, :REC], w["pt"].view(count, REC)), f"{name}: round trip"
        if name in w["outs"]:
            ty, cl = w["outs"][name]
            assert bool((ty == CTYPE).all()) and bool((cl == REC).all()), f"{name}: inner type / content length"
            assert bool((back.view(count, bs)[:, REC] == CTYPE).all()), f"{name}: the type byte"
    cs = w["cts"]["tls13"].numel() // count  # (the bytes between the fragments belong to nobody)
    assert torch.equal(w["cts"]["tls13"].view(count, cs)[:, :REC + 17], w["cts"]["tls13_classes"].view(count, cs)[:, :REC + 17]), \
        "the routed and the class-only images differ"
    assert routes["tls13_seal"] == routes["tls13_open"] == 1 and routes["tls13_classes_seal"] == routes["tls13_classes_open"] == 0
    out = {"batch": w["desc"], "payload_bytes": w["payload"]}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["payload"])
    kept = True
    for d in ("seal", "open"):
        out[f"routed_vs_classes_{d}"] = round(out[f"tls13_{d}"]["ms"] / out[f"tls13_classes_{d}"]["ms"], 4)
        out[f"routed_vs_rfc7905_{d}"] = round(out[f"tls13_{d}"]["ms"] / out[f"rfc7905_{d}"]["ms"], 4)
        spread = max(out[f"tls13_{d}"]["spread"], out[f"tls13_classes_{d}"]["spread"])
        kept = kept and out[f"routed_vs_classes_{d}"] < 1.0 - spread
    out["route_kept"] = kept
    out["routes"] = routes
    # where the time goes: keying pre-pass and record kernel of the two routed calls
    out["timing"] = {}
    for name in ("rfc7905", "tls13"):
        t13 = name != "rfc7905"
        B.set_timing(True)
        for _ in range(5):
            (B.seal_tls13 if t13 else B.seal)(w["legs"][name][0])
            (B.open_tls13 if t13 else B.open_)(w["legs"][name][1])
        torch.cuda.synchronize()
        t = B.timing_read()
        B.set_timing(False)
        out["timing"][name] = {k: round(v, 5) for k, v in t.items() if k.endswith("_ms")}
    return out


def check(w: dict) -> dict:
    """A sample of the routed leg's sealed records against tests/tls13_ref.py."""
    import rfc8439_ref as R
    import tls13_ref as T

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        key, iv, seq, content, frag = w["record"](i)
        assert frag == T.seal(key, iv, seq, content, CTYPE), f"record {i} differs from the TLS 1.3 reference"
    ossl = R.openssl()
    if ossl is not None:
        key, iv, seq, content, frag = w["record"](idx[-1])
        assert frag == ossl.seal(key, T.nonce(iv, seq), T.inner(content, CTYPE), T.header(REC + 17)), "record differs from OpenSSL"
    return {"records_checked": len(idx), "openssl": ossl.version if ossl else None,
            "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 18)
    ap.add_argument("--reps", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", type=Path, default=None, help="also write the JSON here")
    args = ap.parse_args()

    res, bus = ab_legs.prelude("tls13_batch_bench", args.reps, args.warmup)
    w = make(args.records)
    with ab_legs.clock(bus) as res["clock"]:
        res["uniform"] = run(w, args.reps, args.warmup)
    res["uniform"]["check"] = check(w)
    line = json.dumps(res)
    if args.out:
        args.out.write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
