#!/usr/bin/env python3
"""Rate of the long-message path (sg_seal_msg_dev / sg_open_msg_dev) next to the
batch calls on the same bytes.  Prints one JSON line.

Per size (1 MiB, 64 MiB, 1 GiB of device-resident data, 13 bytes of AD):

* ``msg``: one message of n bytes; seal and open time from HIP events around
  each call, median of ``--reps`` launches after ``--warmup``; GiB/s = n / t and
  the HBM roofline fraction (2 n + 16 + adlen) / t against 8 TB/s; the sealed
  bytes and tag are checked against the CPU oracle once per size.
* ``batch_ls0`` / ``batch_ls1``: sg_seal_batch / sg_open_batch on the same bytes
  as n / 16,384 uniform 16 KiB TLS records with sg_set_lockstep(0) (size-class
  kernels) and sg_set_lockstep(1) (wave-per-record kernel).

With ``--rfc8439`` a second message leg, ``msg_rfc_seal`` / ``msg_rfc_open``
(SG_MSG_RFC8439: 12-byte nonce, padded MAC stream), runs beside the draft leg
at the same sizes, checked once per size against OpenSSL's
EVP "ChaCha20-Poly1305" where libcrypto loads (``rfc_check``), and
``rfc_vs_draft_*`` is its time over the draft leg's.

The legs alternate launch by launch in one process, so they share the clock
the board holds; every round runs them in another order (a seeded shuffle,
tools/ab_legs.py), so that no leg always follows the same one.  ``spread`` of a leg is (max - min) / median over its repeats:
the yardstick for "no slower than the lockstep-0 leg" at 1 GiB.

    python tools/msg_bench.py [--sizes 1048576,67108864,1073741824] [--reps 25] [--groups 0] [--rfc8439]
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

HBM_BYTES_PER_S = 8e12
REC = 16384
ADLEN = 13
NONCE12 = bytes([0xC1, 0x52, 0xE3, 0x74, 9, 8, 7, 6, 5, 4, 3, 2])


def summary(ms: list, n: int, traffic: int) -> dict:
    out = ab_legs.summary(ms, n)
    out["hbm_fraction"] = round(traffic / (out["ms"] * 1e-3) / HBM_BYTES_PER_S, 4)
    return out


def run_size(n: int, reps: int, warmup: int, rfc8439: bool = False) -> dict:
    import torch

    from suruga_amd import _native as N
    from suruga_amd import batch as B
    from suruga_amd import msg

    lib = N.load()
    count = n // REC
    assert count * REC == n, "sizes are multiples of 16 KiB (the comparison legs' record size)"
    key = bytes(range(32))
    nonce = bytes([9, 8, 7, 6, 5, 4, 3, 2])
    ad = bytes(range(ADLEN))
    key_t = torch.tensor(list(key), dtype=torch.uint8, device="cuda")
    keys = key_t.view(1, 32)
    ad_t = torch.tensor(list(ad), dtype=torch.uint8, device="cuda")
    pt = torch.empty(n, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, REC, REC, count, 0x6D7367)
    ct = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    back = torch.empty(n, dtype=torch.uint8, device="cuda")
    ct_b = torch.empty(count * (REC + 16), dtype=torch.uint8, device="cuda")
    back_b = torch.empty(n, dtype=torch.uint8, device="cuda")
    st = torch.zeros(1, dtype=torch.uint8, device="cuda")
    st_b = torch.zeros(count, dtype=torch.uint8, device="cuda")
    ws = torch.empty(msg.workspace_size(), dtype=torch.uint8, device="cuda")
    ws_b = torch.empty(B.workspace_size(count), dtype=torch.uint8, device="cuda")

    seal_b = B.Batch(count=count, keys=keys, inp=pt, out=ct_b, uniform_len=REC, in_stride=REC, out_stride=REC + 16,
                     workspace=ws_b)
    open_b = B.Batch(count=count, keys=keys, inp=ct_b, out=back_b, uniform_len=REC + 16, in_stride=REC + 16,
                     out_stride=REC, status=st_b, workspace=ws_b)

    def lockstep(v):
        def set_():
            lib.sg_set_lockstep(v)
        return set_

    legs = {
        "msg_seal": (None, lambda: msg.seal_msg(key_t, nonce, pt, ct, ad=ad_t, workspace=ws)),
        "batch_ls0_seal": (lockstep(0), lambda: B.seal(seal_b)),
        "batch_ls1_seal": (lockstep(1), lambda: B.seal(seal_b)),
        "msg_open": (None, lambda: msg.open_(key_t, nonce, ct, back, st, ad=ad_t, workspace=ws)),
        "batch_ls0_open": (lockstep(0), lambda: B.open_(open_b)),
        "batch_ls1_open": (lockstep(1), lambda: B.open_(open_b)),
    }
    if rfc8439:
        ct_r = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
        back_r = torch.empty(n, dtype=torch.uint8, device="cuda")
        st_r = torch.zeros(1, dtype=torch.uint8, device="cuda")
        legs["msg_rfc_seal"] = (None, lambda: msg.seal_msg(key_t, NONCE12, pt, ct_r, ad=ad_t, workspace=ws,
                                                            rfc8439=True))
        legs["msg_rfc_open"] = (None, lambda: msg.open_(key_t, NONCE12, ct_r, back_r, st_r, ad=ad_t, workspace=ws,
                                                        rfc8439=True))
    prev = lib.sg_set_lockstep(-1)
    try:
        times = ab_legs.timed_legs(legs, reps, warmup)
    finally:
        lib.sg_set_lockstep(prev)
    assert int(st.item()) == 0 and int(st_b.sum().item()) == 0, "open status"
    assert torch.equal(back, pt) and torch.equal(back_b, pt), "round trip"
    if rfc8439:
        assert int(st_r.item()) == 0 and torch.equal(back_r, pt), "RFC 8439 round trip"

    out = {"n": n, "adlen": ADLEN, "plan": msg.plan_for(n, ADLEN, max(msg.set_groups(-1), 0))}
    for name, ms in times.items():
        out[name] = summary(ms, n, 2 * n + 16 + ADLEN)
    for d in ("seal", "open"):
        out[f"msg_vs_ls0_{d}"] = round(out[f"msg_{d}"]["ms"] / out[f"batch_ls0_{d}"]["ms"], 4)
        if rfc8439:
            out[f"rfc_vs_draft_{d}"] = round(out[f"msg_rfc_{d}"]["ms"] / out[f"msg_{d}"]["ms"], 4)
    return out


def check_size(n: int) -> dict:
    """One seal of the size's message against the CPU oracle (every byte and the tag)."""
    import torch

    from oracle_ffi import oracle
    from suruga_amd import batch as B
    from suruga_amd import msg

    key, nonce, ad = bytes(range(32)), bytes([9, 8, 7, 6, 5, 4, 3, 2]), bytes(range(ADLEN))
    key_t = torch.tensor(list(key), dtype=torch.uint8, device="cuda")
    ad_t = torch.tensor(list(ad), dtype=torch.uint8, device="cuda")
    pt = torch.empty(n, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, REC, REC, n // REC, 0x6D7367)
    ct = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    msg.seal_msg(key_t, nonce, pt, ct, ad=ad_t)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = oracle().seal(key, nonce, pt.cpu().numpy().tobytes(), ad)
    secs = time.perf_counter() - t0
    got = ct.cpu().numpy().tobytes()
    res = {"oracle_s": round(secs, 2), "tag_ok": got[-16:] == want[-16:], "ct_ok": got == want}
    assert res["tag_ok"] and res["ct_ok"], "message differs from the oracle"
    return res


def check_size_rfc8439(n: int) -> dict:
    """One RFC 8439 seal of the size's message against OpenSSL (every byte and the tag)."""
    import torch

    import rfc8439_ref
    from suruga_amd import batch as B
    from suruga_amd import msg

    ossl = rfc8439_ref.openssl()
    if ossl is None:
        return {"openssl": None}
    key, ad = bytes(range(32)), bytes(range(ADLEN))
    key_t = torch.tensor(list(key), dtype=torch.uint8, device="cuda")
    ad_t = torch.tensor(list(ad), dtype=torch.uint8, device="cuda")
    pt = torch.empty(n, dtype=torch.uint8, device="cuda")
    B.fill_records(pt, REC, REC, n // REC, 0x6D7367)
    ct = torch.empty(n + 16, dtype=torch.uint8, device="cuda")
    msg.seal_msg(key_t, NONCE12, pt, ct, ad=ad_t, rfc8439=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    want = ossl.seal(key, NONCE12, pt.cpu().numpy().tobytes(), ad)
    secs = time.perf_counter() - t0
    got = ct.cpu().numpy().tobytes()
    res = {"openssl": ossl.version, "openssl_s": round(secs, 2), "tag_ok": got[-16:] == want[-16:], "ct_ok": got == want}
    assert res["tag_ok"] and res["ct_ok"], "RFC 8439 message differs from OpenSSL"
    return res


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--sizes", default="1048576,67108864,1073741824")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--groups", type=int, default=None, help="sg_set_msg_groups (default: leave the setting)")
    ap.add_argument("--no-check", action="store_true", help="skip the oracle comparison")
    ap.add_argument("--rfc8439", action="store_true", help="add the RFC 8439 message leg beside the draft leg")
    args = ap.parse_args()
    if args.reps < 20:
        ap.error("--reps must be at least 20")

    from suruga_amd import msg

    res, bus = ab_legs.prelude("msg_bench", args.reps, args.warmup)
    if args.groups is not None:
        msg.set_groups(args.groups)
    sizes = [int(s) for s in args.sizes.split(",")]
    res.update(msg_groups=msg.set_groups(-1), sizes=[])
    for n in sizes:
        # the clock the board holds while the largest size is timed; the oracle check runs apart from it
        with ab_legs.clock(bus, n == max(sizes)) as clk:
            r = run_size(n, args.reps, args.warmup, args.rfc8439)
        if clk:
            res["clock"] = clk
        if not args.no_check:
            r.update(check_size(n))
            if args.rfc8439:
                r["rfc_check"] = check_size_rfc8439(n)
        res["sizes"].append(r)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
