#!/usr/bin/env python3
"""Rate of the WireGuard transport data batch (sg_seal_batch_wg / sg_open_batch_wg) beside
its sibling kernel and beside the AEAD share a WireGuard caller could get from the library
before.  Prints one JSON line and writes it to profiles/wg_bench.json.

The batch: ``--packets`` (default 2^20) inner packets of 256 sessions, inner lengths uniform
in 1,200..1,452 bytes (what tools/quic_bench.py draws), each starting with an IPv4 header
that states its length, lying back to back at whatever address that gives them; pad_cap 0,
so every message carries its inner packet rounded up to 16 bytes.  Four pairs of legs in
one process:

* ``wg_seal`` / ``wg_open``: the transport data calls, separate input and output buffers --
  header, padding, counter and inner length on the device;
* ``wg_inplace_seal`` / ``wg_inplace_open``: the same calls in place (seal out + 16 == in,
  open out == in + 16); the buffer is put back to its start image ahead of every timed launch;
* ``quic_seal`` / ``quic_open``: ``sg_*_batch_quic`` over payloads of the same (padded)
  lengths behind an 11-byte header -- the sibling kernel, which does strictly more a packet:
  one more ChaCha20 block (the header protection mask) and an AD;
* ``rfc_seal`` / ``rfc_open``: ``sg_*_batch_rfc8439`` in explicit mode with an empty AD over
  payloads padded on the host, with 12-byte nonces built on the host: what a WireGuard caller
  had before.  It is the AEAD only: no header is written or checked, no counter read, no
  inner length found, and the host's nonce and padding work is NOT in its number.

The legs alternate launch by launch, every round in another order (a seeded shuffle,
tools/ab_legs.py); each reports the median of ``--reps`` launches after ``--warmup`` from
HIP events, GiB/s of AEAD payload and ``spread`` = (max - min) / median.  The ``*_vs_*``
figures are a WireGuard leg's time over the other leg's: figures to report, not bounds --
nothing else in the library produces the WireGuard legs' output.  A sample of messages is
compared with tests/wg_ref.py, every byte; every packet must open with its counter and its
inner length and round-trip.

    python tools/wg_bench.py [--packets 1048576] [--reps 25]
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

SEED = 0x77677470
SAMPLE = 24
SESSIONS = 256
LO, HI = 1200, 1452
Q_PN_OFF, Q_PN_LEN = 9, 2
Q_HDR = Q_PN_OFF + Q_PN_LEN
Q_FIRST = 0x40 | (Q_PN_LEN - 1)


def make(count: int):
    import numpy as np
    import torch

    from suruga_amd import batch as B
    from suruga_amd import quic as QU
    from suruga_amd import wg as WG

    rng = np.random.default_rng(SEED)
    ilen = rng.integers(LO, HI + 1, size=count).astype(np.uint32)        # inner lengths
    plen = (ilen + np.uint32(15)) // np.uint32(16) * np.uint32(16)       # padded: the AEAD's bytes
    mlen = plen + np.uint32(32)
    cum = lambda a: np.concatenate([[0], np.cumsum(a[:-1], dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
    raw_off, msg_off = cum(plen), cum(mlen)
    raw_bytes, msg_bytes = int(raw_off[-1] + plen[-1]), int(msg_off[-1] + mlen[-1])
    kidx_h = rng.integers(0, SESSIONS, size=count).astype(np.uint32)
    ctr_h = rng.integers(0, 2**40, size=count).astype(np.uint64)
    keys_h = rng.integers(0, 256, 32 * SESSIONS, dtype=np.uint8).tobytes()
    recv_h = rng.integers(0, 2**32, size=SESSIONS, dtype=np.uint64).astype(np.uint32)
    t8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")  # noqa: E731
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")  # noqa: E731
    empty = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")  # noqa: E731

    # the inner packets, each in a slot of its padded length; the bytes behind an inner packet are not zero
    raw = empty(raw_bytes)
    B.fill_records(raw, 0, raw_bytes, 1, SEED)
    d_raw_off, d_msg_off = t64(raw_off), t64(msg_off)
    raw[d_raw_off] = 0x45
    raw[d_raw_off + 2] = t8((ilen >> np.uint32(8)).astype(np.uint8).tobytes())
    raw[d_raw_off + 3] = t8(ilen.astype(np.uint8).tobytes())
    msg, back = empty(msg_bytes), empty(raw_bytes)
    st = torch.full((4, count), 0xFF, dtype=torch.uint8, device="cuda")
    ctr = t64(ctr_h)
    ctr_out = torch.zeros((2, count), dtype=torch.int64, device="cuda")
    ilen_out = torch.zeros((2, count), dtype=torch.int32, device="cuda")
    keys, kidx = t8(keys_h), t32(kidx_h)
    tables = dict(count=count, keys=keys, key_index=kidx)
    d_ilen, d_mlen = t32(ilen), t32(mlen)
    wg = (WG.WgBatch(inp=raw, out=msg, status=st[0], receiver=t32(recv_h), counter=ctr, lens=d_ilen, max_len=HI,
                     in_off=d_raw_off, out_off=d_msg_off, **tables),
          WG.WgBatch(inp=msg, out=back, status=st[1], counter_out=ctr_out[0], inner_len=ilen_out[0], lens=d_mlen,
                     max_len=int(mlen.max()), in_off=d_msg_off, out_off=d_raw_off, **tables))
    # in place: one buffer of message slots, the inner packet 16 bytes into its slot
    place = empty(msg_bytes + 16)
    start = torch.zeros(msg_bytes + 16, dtype=torch.uint8, device="cuda")
    idx = torch.arange(int(plen.max()), device="cuda")
    for lo in range(0, count, 1 << 16):  # copy the inner packets over, some 2^16 at a time
        hi = min(count, lo + (1 << 16))
        L = torch.from_numpy(ilen[lo:hi].astype(np.int64)).to("cuda")
        keep = idx[None, :] < L[:, None]
        src = (d_raw_off[lo:hi, None] + idx[None, :])[keep]
        dst = (d_msg_off[lo:hi, None] + 16 + idx[None, :])[keep]
        start[dst] = raw[src]
    sealed = empty(msg_bytes + 16)
    wgp = (WG.WgBatch(inp=place[16:], out=place, status=st[2], receiver=wg[0].receiver, counter=ctr, lens=d_ilen, max_len=HI,
                      in_off=d_msg_off, out_off=d_msg_off, **tables),
           WG.WgBatch(inp=place, out=place[16:], status=st[3], counter_out=ctr_out[1], inner_len=ilen_out[1], lens=d_mlen,
                      max_len=int(mlen.max()), in_off=d_msg_off, out_off=d_msg_off, **tables))

    # the sibling: QUIC packets whose payload has the padded length
    q_raw_len = plen + np.uint32(Q_HDR)
    q_raw_off, q_prot_off = cum(q_raw_len), cum(q_raw_len + np.uint32(16))
    q_raw_bytes, q_prot_bytes = int(q_raw_off[-1] + q_raw_len[-1]), int(q_prot_off[-1] + q_raw_len[-1] + 16)
    q_raw = empty(q_raw_bytes)
    B.fill_records(q_raw, 0, q_raw_bytes, 1, SEED + 1)
    dq_raw_off, dq_prot_off = t64(q_raw_off), t64(q_prot_off)
    q_raw[dq_raw_off] = Q_FIRST
    q_prot, q_back = empty(q_prot_bytes), empty(q_raw_bytes)
    q_st = torch.full((2, count), 0xFF, dtype=torch.uint8, device="cuda")
    q_pn_out = torch.zeros(count, dtype=torch.int64, device="cuda")
    ivs_h, hps_h = (rng.integers(0, 256, w * SESSIONS, dtype=np.uint8).tobytes() for w in (12, 32))
    q_tables = dict(count=count, keys=keys, ivs=t8(ivs_h), hp_keys=t8(hps_h), key_index=kidx, uniform_pn_off=Q_PN_OFF, pn=ctr)
    quic = (QU.QuicBatch(inp=q_raw, out=q_prot, status=q_st[0], lens=t32(q_raw_len), max_len=int(q_raw_len.max()),
                         in_off=dq_raw_off, out_off=dq_prot_off, **q_tables),
            QU.QuicBatch(inp=q_prot, out=q_back, status=q_st[1], pn_out=q_pn_out, lens=t32(q_raw_len + np.uint32(16)),
                         max_len=int(q_raw_len.max()) + 16, in_off=dq_prot_off, out_off=dq_raw_off, **q_tables))

    # the AEAD alone, as before: payloads padded and nonces built on the host (neither is timed)
    nonces = np.zeros((count, 12), dtype=np.uint8)
    nonces[:, 4:] = ctr_h.astype("<u8").view(np.uint8).reshape(count, 8)
    r_ct_off = cum(plen + np.uint32(16))
    r_ct_bytes = int(r_ct_off[-1] + plen[-1] + 16)
    r_pt = torch.zeros(raw_bytes, dtype=torch.uint8, device="cuda")
    for lo in range(0, count, 1 << 16):
        hi = min(count, lo + (1 << 16))
        L = torch.from_numpy(ilen[lo:hi].astype(np.int64)).to("cuda")
        at = (d_raw_off[lo:hi, None] + idx[None, :])[idx[None, :] < L[:, None]]
        r_pt[at] = raw[at]
    r_ct, r_back = empty(r_ct_bytes), empty(raw_bytes)
    r_st = torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = empty(B.workspace_size(count))
    common = dict(count=count, keys=keys.view(SESSIONS, 32), key_index=kidx, tls=False, rfc8439=True,
                  nonces=t8(nonces.tobytes()), ads=torch.zeros(count, dtype=torch.uint8, device="cuda"), ad_len=0, ad_stride=1,
                  workspace=ws)
    d_ct_off = t64(r_ct_off)
    rfc = (B.Batch(inp=r_pt, out=r_ct, lens=t32(plen), max_len=int(plen.max()), in_off=d_raw_off, out_off=d_ct_off, **common),
           B.Batch(inp=r_ct, out=r_back, lens=t32(plen + np.uint32(16)), max_len=int(plen.max()) + 16, in_off=d_ct_off,
                   out_off=d_raw_off, status=r_st, **common))

    raw_host = raw.cpu().numpy()

    def packet(i, buf):  # (key, receiver, counter, inner, the message in buf) of packet i
        k, o, q = int(kidx_h[i]), int(raw_off[i]), int(msg_off[i])
        return (keys_h[32 * k:32 * k + 32], int(recv_h[k]), int(ctr_h[i]), raw_host[o:o + int(ilen[i])].tobytes(),
                buf[q:q + int(mlen[i])].cpu().numpy().tobytes())

    return dict(count=count, payload=int(plen.sum()), wg=wg, wgp=wgp, quic=quic, rfc=rfc, raw=raw, msg=msg, back=back,
                place=place, start=start, sealed=sealed, st=st, ctr=ctr, ctr_out=ctr_out, ilen=d_ilen, ilen_out=ilen_out,
                q_st=q_st, q_pn_out=q_pn_out, r_st=r_st, r_pt=r_pt, r_back=r_back, r_ct=r_ct, packet=packet,
                raw_off=d_raw_off, msg_off=d_msg_off, ct_off=d_ct_off, min_len=int(ilen.min()),
                desc=f"{count} inner packets, lengths {LO}..{HI} (mean {ilen.mean():.0f} B, padded {plen.mean():.0f} B), "
                     f"{SESSIONS} sessions, pad_cap 0")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import batch as B
    from suruga_amd import quic as QU
    from suruga_amd import wg as WG

    # the in-place legs' start images: the inner packets in their slots, and their sealed form
    w["place"].copy_(w["start"])
    WG.seal_wg(w["wgp"][0])
    w["sealed"].copy_(w["place"])
    legs = {"wg_seal": lambda: WG.seal_wg(w["wg"][0]), "wg_open": lambda: WG.open_wg(w["wg"][1]),
            "wg_inplace_seal": (lambda: w["place"].copy_(w["start"]), lambda: WG.seal_wg(w["wgp"][0])),
            "wg_inplace_open": (lambda: w["place"].copy_(w["sealed"]), lambda: WG.open_wg(w["wgp"][1])),
            "quic_seal": lambda: QU.seal_quic(w["quic"][0]), "quic_open": lambda: QU.open_quic(w["quic"][1]),
            "rfc_seal": lambda: B.seal(w["rfc"][0]), "rfc_open": lambda: B.open_(w["rfc"][1])}
    # one pass in order first, so that every open leg has its input
    for name in ("wg_seal", "wg_open", "quic_seal", "quic_open", "rfc_seal", "rfc_open"):
        legs[name]()
    times = ab_legs.timed_legs(legs, reps, warmup)
    w["place"].copy_(w["sealed"])  # whichever in-place leg ran last: leave the opened image behind
    WG.open_wg(w["wgp"][1])
    torch.cuda.synchronize()
    for s in (w["st"], w["q_st"], w["r_st"]):
        assert int(s.sum().item()) == 0, "status"
    for k in (0, 1):
        assert torch.equal(w["ctr_out"][k], w["ctr"]) and torch.equal(w["ilen_out"][k], w["ilen"]), "counters and inner lengths"
    assert torch.equal(w["q_pn_out"], w["ctr"]), "packet numbers"
    # the round trip -- every packet's first, second and (of the shortest) last inner byte -- and the three
    # constructions agree on the ciphertext
    ro, mo, co = w["raw_off"], w["msg_off"], w["ct_off"]
    for d in (0, 1, w["min_len"] - 1):
        want = w["raw"][ro + d]
        assert torch.equal(w["back"][ro + d], want) and torch.equal(w["place"][mo + 16 + d], want), "round trip"
        assert torch.equal(w["r_back"][ro + d], want), "round trip (rfc)"
    for d in (0, 7, 1000):
        assert torch.equal(w["msg"][mo + 16 + d], w["r_ct"][co + d]) and torch.equal(w["sealed"][mo + 16 + d], w["r_ct"][co + d])
    out = {"batch": w["desc"], "payload_bytes": w["payload"]}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["payload"])
        out[name]["mpps"] = round(w["count"] / (out[name]["ms"] * 1e-3) / 1e6, 1)
    for d in ("seal", "open"):
        for a in ("wg", "wg_inplace"):
            for b in ("quic", "rfc"):
                out[f"{a}_vs_{b}_{d}"] = round(out[f"{a}_{d}"]["ms"] / out[f"{b}_{d}"]["ms"], 4)
    out["rfc_legs"] = "AEAD only; the host's nonce and padding work is not in their number"
    return out


def check(w: dict) -> dict:
    """A sample of messages, of both seal legs, against tests/wg_ref.py, and back."""
    import wg_ref as W

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        for buf in (w["msg"], w["sealed"]):
            key, receiver, counter, inner, got = w["packet"](i, buf)
            assert got == W.protect(key, receiver, counter, inner), f"message {i} differs from the reference"
            pad = bytes(len(got) - 32 - len(inner))
            assert W.unprotect(key, got) == (0, inner + pad, counter, len(inner))
    return {"packets_checked": len(idx), "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wg_bench.json"), help="where the JSON goes ('' : nowhere)")
    args = ap.parse_args()
    assert args.reps >= 25 or args.out == "", "a recorded run takes at least 25 rounds"

    res, bus = ab_legs.prelude("wg_bench", args.reps, args.warmup)
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
