#!/usr/bin/env python3
"""Rate of the QUIC packet protection batch (sg_seal_batch_quic / sg_open_batch_quic)
beside the AEAD share a QUIC caller could get from the library before.  Prints one JSON
line and writes it to profiles/quic_bench.json.

The batch: ``--packets`` (default 2^20) short-header 1-RTT packets of 256 connections,
protected lengths uniform in 1,200..1,452 bytes, an 8-byte connection ID and a 2-byte
packet number (pn_off 9, header 11 bytes), lying back to back at whatever address that
gives them.  Four legs in one process:

* ``quic_seal`` / ``quic_open``: the packet protection calls -- header protection, packet
  number, nonce and AD on the device;
* ``rfc_seal`` / ``rfc_open``: ``sg_*_batch_rfc8439`` in explicit mode over the same payload
  bytes, with 12-byte nonces and the 11-byte headers as a uniform AD in arrays of their own,
  which a caller had to build on the host; no header protection.

The legs alternate launch by launch, every round in another order (a seeded shuffle,
tools/ab_legs.py); each reports the median of ``--reps`` launches after ``--warmup`` from
HIP events, GiB/s of payload and ``spread`` = (max - min) / median.  ``quic_vs_rfc_*`` is
the QUIC time over the RFC time: a figure to report, not a bound -- nothing else in the
library produces the QUIC legs' output.  A sample of protected packets is compared with
tests/quic_ref.py, every byte; every packet must open and round-trip.

    python tools/quic_bench.py [--packets 1048576] [--reps 25]
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

SEED = 0x71756963
SAMPLE = 24
CONNS = 256
PN_OFF, PN_LEN = 9, 2
HDR = PN_OFF + PN_LEN
FIRST = 0x40 | (PN_LEN - 1)
LO, HI = 1200, 1452


def make(count: int):
    import numpy as np
    import torch

    from suruga_amd import batch as B
    from suruga_amd import quic as QU

    rng = np.random.default_rng(SEED)
    plen = rng.integers(LO, HI + 1, size=count).astype(np.uint32)       # protected lengths
    raw_len = plen - 16
    n = raw_len - HDR                                                    # payload lengths
    raw_off = np.concatenate([[0], np.cumsum(raw_len[:-1], dtype=np.uint64)]).astype(np.uint64)
    prot_off = np.concatenate([[0], np.cumsum(plen[:-1], dtype=np.uint64)]).astype(np.uint64)
    raw_bytes, prot_bytes = int(raw_off[-1] + raw_len[-1]), int(prot_off[-1] + plen[-1])
    kidx_h = rng.integers(0, CONNS, size=count).astype(np.uint32)
    pn_h = (rng.integers(0, 2**40, size=count).astype(np.uint64))
    keys_h, ivs_h, hps_h = (rng.integers(0, 256, w * CONNS, dtype=np.uint8).tobytes() for w in (32, 12, 32))
    t8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")  # noqa: E731
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")  # noqa: E731

    raw = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda")
    B.fill_records(raw, 0, raw_bytes, 1, SEED)
    raw[t64(raw_off)] = FIRST  # a short header with a 2-byte packet number
    prot = torch.empty(prot_bytes, dtype=torch.uint8, device="cuda")
    back = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda")
    st = torch.full((2, count), 0xFF, dtype=torch.uint8, device="cuda")
    pn, pn_out = t64(pn_h), torch.zeros(count, dtype=torch.int64, device="cuda")
    tables = dict(keys=t8(keys_h), ivs=t8(ivs_h), hp_keys=t8(hps_h), key_index=t32(kidx_h), uniform_pn_off=PN_OFF)
    d_raw_off, d_prot_off = t64(raw_off), t64(prot_off)
    quic = (QU.QuicBatch(count=count, inp=raw, out=prot, status=st[0], pn=pn, lens=t32(raw_len), max_len=HI - 16,
                         in_off=d_raw_off, out_off=d_prot_off, **tables),
            QU.QuicBatch(count=count, inp=prot, out=back, status=st[1], pn=pn, pn_out=pn_out, lens=t32(plen), max_len=HI,
                         in_off=d_prot_off, out_off=d_raw_off, **tables))

    # the AEAD alone, as before: nonces and ADs built on the host, in arrays of their own
    iv = np.frombuffer(ivs_h, dtype=np.uint8).reshape(CONNS, 12)[kidx_h].copy()
    iv[:, 4:] ^= pn_h.astype(">u8").view(np.uint8).reshape(count, 8)
    raw_host = raw.cpu().numpy()
    ads = np.stack([raw_host[raw_off + np.uint64(i)] for i in range(HDR)], axis=1)
    ads[:, PN_OFF] = (pn_h >> np.uint64(8)).astype(np.uint8)
    ads[:, PN_OFF + 1] = pn_h.astype(np.uint8)
    rct = torch.empty(prot_bytes, dtype=torch.uint8, device="cuda")
    rback = torch.empty(raw_bytes, dtype=torch.uint8, device="cuda")
    rst = torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = torch.empty(B.workspace_size(count), dtype=torch.uint8, device="cuda")
    common = dict(count=count, keys=tables["keys"].view(CONNS, 32), key_index=tables["key_index"], tls=False, rfc8439=True,
                  nonces=t8(iv.tobytes()), ads=t8(ads.tobytes()), ad_len=HDR, ad_stride=HDR, workspace=ws)
    pay_off, ct_off = t64(raw_off + np.uint64(HDR)), t64(prot_off + np.uint64(HDR))
    rfc = (B.Batch(inp=raw, out=rct, lens=t32(n), max_len=int(n.max()), in_off=pay_off, out_off=ct_off, **common),
           B.Batch(inp=rct, out=rback, lens=t32(n + 16), max_len=int(n.max()) + 16, in_off=ct_off, out_off=pay_off,
                   status=rst, **common))

    def packet(i):  # (key, iv, hp, pn, raw, pn_off, protected) of packet i
        k, o, q = int(kidx_h[i]), int(raw_off[i]), int(prot_off[i])
        return (keys_h[32 * k:32 * k + 32], ivs_h[12 * k:12 * k + 12], hps_h[32 * k:32 * k + 32], int(pn_h[i]),
                raw_host[o:o + int(raw_len[i])].tobytes(), PN_OFF, prot[q:q + int(plen[i])].cpu().numpy().tobytes())

    return dict(count=count, payload=int(n.sum()), quic=quic, rfc=rfc, raw=raw, prot=prot, back=back, st=st, pn=pn,
                pn_out=pn_out, rct=rct, rback=rback, rst=rst, packet=packet, pay_off=(raw_off + np.uint64(HDR), n),
                prot_off=(prot_off + np.uint64(HDR), n),
                desc=f"{count} short-header packets, protected lengths {LO}..{HI} (mean payload {n.mean():.0f} B), "
                     f"{CONNS} connections, pn_off {PN_OFF}, pn_len {PN_LEN}")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import batch as B
    from suruga_amd import quic as QU

    legs = {"quic_seal": lambda: QU.seal_quic(w["quic"][0]), "quic_open": lambda: QU.open_quic(w["quic"][1]),
            "rfc_seal": lambda: B.seal(w["rfc"][0]), "rfc_open": lambda: B.open_(w["rfc"][1])}
    times = ab_legs.timed_legs(legs, reps, warmup)
    assert int(w["st"].sum().item()) == 0 and int(w["rst"].sum().item()) == 0, "status"
    assert torch.equal(w["pn_out"], w["pn"]), "packet numbers"
    # the round trip: headers (their packet number fields now written) and payloads
    first = w["back"][:HDR].cpu().numpy().tobytes()
    assert first[0] == FIRST and first[1:PN_OFF] == w["raw"][1:PN_OFF].cpu().numpy().tobytes()
    idx = torch.from_numpy(w["pay_off"][0].view("int64")).to("cuda")
    for d in (0, 1, int(w["pay_off"][1].min()) - 1):  # every packet's first, second and (of the shortest) last payload byte
        assert torch.equal(w["back"][idx + d], w["raw"][idx + d]) and torch.equal(w["rback"][idx + d], w["raw"][idx + d])
    cidx = torch.from_numpy(w["prot_off"][0].view("int64")).to("cuda")
    for d in (0, 7, 1000):  # the two constructions agree on the ciphertext
        assert torch.equal(w["prot"][cidx + d], w["rct"][cidx + d]), "ciphertext"
    out = {"batch": w["desc"], "payload_bytes": w["payload"]}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["payload"])
        out[name]["mpps"] = round(w["count"] / (out[name]["ms"] * 1e-3) / 1e6, 1)
    for d in ("seal", "open"):
        out[f"quic_vs_rfc_{d}"] = round(out[f"quic_{d}"]["ms"] / out[f"rfc_{d}"]["ms"], 4)
    return out


def check(w: dict) -> dict:
    """A sample of protected packets against tests/quic_ref.py, and back."""
    import quic_ref as Q

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        key, iv, hp, pn, raw, pn_off, got = w["packet"](i)
        assert got == Q.protect(key, iv, hp, pn, raw, pn_off), f"packet {i} differs from the reference"
        rc, body, num = Q.unprotect(key, iv, hp, pn, got, pn_off)
        assert (rc, num) == (0, pn) and body[HDR:] == raw[HDR:]
    return {"packets_checked": len(idx), "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quic_bench.json"), help="where the JSON goes ('' : nowhere)")
    args = ap.parse_args()
    assert args.reps >= 25 or args.out == "", "a recorded run takes at least 25 rounds"

    res, bus = ab_legs.prelude("quic_bench", args.reps, args.warmup)
    w = make(args.packets)
    with ab_legs.clock(bus) as res["clock"]:
        res.update(run(w, args.reps, args.warmup))
    res["check"] = check(w)
    res["measured_by"] = "builder-run"
    line = json.dumps(res)
    if args.out:
        Path(args.out).write_text(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
