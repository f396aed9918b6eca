#!/usr/bin/env python3
"""Rate of the IPsec ESP batch (sg_seal_batch_esp / sg_open_batch_esp) beside its sibling
kernel and beside the AEAD share an ESP caller could get from the library before.  Prints
one JSON line and writes it to profiles/esp_bench.json.

The batch: ``--packets`` (default 2^20) payloads of 256 SAs, lengths uniform in 1,200..1,452
bytes (what tools/wg_bench.py draws), lying back to back at whatever address that gives
them; align 4, extended sequence numbers on (12-byte AD, the high half inferred on open),
per-packet next headers, the IV the sequence number.  Four pairs of legs in one process:

* ``esp_seal`` / ``esp_open``: the ESP calls, separate input and output buffers -- header,
  nonce, AD, padding and trailer on seal; SPI check, sequence number, ICV and the trailer's
  parse on open, all on the device;
* ``esp_inplace_seal`` / ``esp_inplace_open``: the same calls in place (seal out + 16 == in,
  open out == in + 16); the buffer is put back to its start image ahead of every timed launch;
* ``wg_seal`` / ``wg_open``: ``sg_*_batch_wg`` over inner packets of the same lengths (padded
  to 16 there, so its AEAD runs over slightly more bytes) -- the sibling kernel, which has
  no AD block, at most 15 bytes to make up on seal and two words to look at on open;
* ``rfc_seal`` / ``rfc_open``: ``sg_*_batch_rfc8439`` in explicit mode with a 12-byte AD over
  plaintexts whose trailer was built on the host, with nonces and ADs built on the host:
  what an ESP caller had before.  It is the AEAD only: no header is written or checked, no
  sequence number inferred, no trailer parsed, and the host's work is NOT in its number.

The legs alternate launch by launch, every round in another order (a seeded shuffle,
tools/ab_legs.py); each reports the median of ``--reps`` launches after ``--warmup`` from
HIP events, GiB/s of its own AEAD payload and ``spread`` = (max - min) / median.  The
``*_vs_*`` figures are an ESP leg's time over the other leg's: figures to report beside the
spreads, not bounds -- nothing else in the library produces the ESP legs' output.  A
sample of packets is compared with tests/esp_ref.py, every byte; every packet must open with
its 64-bit sequence number, payload length and next header and round-trip.

    python tools/esp_bench.py [--packets 1048576] [--reps 25]
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

SEED = 0x65737062
SAMPLE = 24
SAS = 256
LO, HI = 1200, 1452
ALIGN = 4
WINDOW = 1 << 22


def make(count: int):
    import numpy as np
    import torch

    from suruga_amd import batch as B
    from suruga_amd import esp as ESP
    from suruga_amd import wg as WG

    rng = np.random.default_rng(SEED)
    u32 = np.uint32
    ilen = rng.integers(LO, HI + 1, size=count).astype(u32)              # payload lengths
    plen = (ilen + u32(2) + u32(ALIGN - 1)) // u32(ALIGN) * u32(ALIGN)   # ESP: payload, padding, trailer
    pad = plen - ilen - u32(2)
    mlen = plen + u32(32)
    wlen = (ilen + u32(15)) // u32(16) * u32(16)                         # WireGuard: padded to 16
    wmlen = wlen + u32(32)
    slot = (ilen + u32(2) + u32(15)) // u32(16) * u32(16)                # a payload's slot holds either padding
    cum = lambda a: np.concatenate([[0], np.cumsum(a[:-1], dtype=np.uint64)]).astype(np.uint64)  # noqa: E731
    raw_off, msg_off, wmsg_off = cum(slot), cum(mlen), cum(wmlen)
    raw_bytes, msg_bytes, wmsg_bytes = int(raw_off[-1] + slot[-1]), int(msg_off[-1] + mlen[-1]), int(wmsg_off[-1] + wmlen[-1])
    kidx_h = rng.integers(0, SAS, size=count).astype(u32)
    # every SA's numbers run across a 2^32 boundary: base + the packet's place in the batch
    base_h = (rng.integers(1, 2**20, size=SAS).astype(np.uint64) << np.uint64(32)) - np.uint64(count // 2)
    seq_h = base_h[kidx_h] + np.arange(count, dtype=np.uint64)
    top_h = base_h + np.uint64(count)
    nh_h = rng.integers(0, 256, size=count, dtype=np.uint8)
    keys_h = rng.integers(0, 256, 32 * SAS, dtype=np.uint8).tobytes()
    salts_h = rng.integers(0, 256, 4 * SAS, dtype=np.uint8)
    spi_h = rng.integers(256, 2**32, size=SAS, dtype=np.uint64).astype(u32)
    t8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")  # noqa: E731
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")  # noqa: E731
    empty = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")  # noqa: E731

    # the payloads, each in its slot; the bytes behind a payload are not a trailer.  An IPv4 header's
    # first four bytes in front, so that the WireGuard legs find their inner length
    raw = empty(raw_bytes)
    B.fill_records(raw, 0, raw_bytes, 1, SEED)
    d_raw_off, d_msg_off, d_wmsg_off = t64(raw_off), t64(msg_off), t64(wmsg_off)
    raw[d_raw_off] = 0x45
    raw[d_raw_off + 2] = t8((ilen >> u32(8)).astype(np.uint8).tobytes())
    raw[d_raw_off + 3] = t8(ilen.astype(np.uint8).tobytes())
    msg, back = empty(msg_bytes), empty(raw_bytes)
    st = torch.full((4, count), 0xFF, dtype=torch.uint8, device="cuda")
    seq, nh = t64(seq_h), t8(nh_h.tobytes())
    seq_out = torch.zeros((2, count), dtype=torch.int64, device="cuda")
    plen_out = torch.zeros((2, count), dtype=torch.int32, device="cuda")
    nh_out = torch.zeros((2, count), dtype=torch.uint8, device="cuda")
    keys, kidx = t8(keys_h), t32(kidx_h)
    tables = dict(count=count, keys=keys, salts=t8(salts_h.tobytes()), spi=t32(spi_h), sa_index=kidx, esn=True)
    recv = dict(replay_top=t64(top_h), window=WINDOW)
    d_ilen, d_mlen = t32(ilen), t32(mlen)
    esp = (ESP.EspBatch(inp=raw, out=msg, status=st[0], seq=seq, next_header=nh, align=ALIGN, lens=d_ilen, max_len=HI,
                        in_off=d_raw_off, out_off=d_msg_off, **tables),
           ESP.EspBatch(inp=msg, out=back, status=st[1], seq_out=seq_out[0], payload_len=plen_out[0], next_header_out=nh_out[0],
                        lens=d_mlen, max_len=int(mlen.max()), in_off=d_msg_off, out_off=d_raw_off, **recv, **tables))
    # in place: one buffer of packet slots, the payload 16 bytes into its slot
    place = empty(msg_bytes + 16)
    start = torch.zeros(msg_bytes + 16, dtype=torch.uint8, device="cuda")
    idx = torch.arange(int(slot.max()), device="cuda")
    for lo in range(0, count, 1 << 16):  # copy the payloads over, some 2^16 at a time
        hi = min(count, lo + (1 << 16))
        L = torch.from_numpy(ilen[lo:hi].astype(np.int64)).to("cuda")
        keep = idx[None, :] < L[:, None]
        src = (d_raw_off[lo:hi, None] + idx[None, :])[keep]
        dst = (d_msg_off[lo:hi, None] + 16 + idx[None, :])[keep]
        start[dst] = raw[src]
    sealed = empty(msg_bytes + 16)
    espp = (ESP.EspBatch(inp=place[16:], out=place, status=st[2], seq=seq, next_header=nh, align=ALIGN, lens=d_ilen, max_len=HI,
                         in_off=d_msg_off, out_off=d_msg_off, **tables),
            ESP.EspBatch(inp=place, out=place[16:], status=st[3], seq_out=seq_out[1], payload_len=plen_out[1],
                         next_header_out=nh_out[1], lens=d_mlen, max_len=int(mlen.max()), in_off=d_msg_off, out_off=d_msg_off,
                         **recv, **tables))

    # the sibling: WireGuard messages of the same inner lengths
    w_msg, w_back = empty(wmsg_bytes), empty(raw_bytes)
    w_st = torch.full((2, count), 0xFF, dtype=torch.uint8, device="cuda")
    w_ctr_out = torch.zeros(count, dtype=torch.int64, device="cuda")
    w_ilen_out = torch.zeros(count, dtype=torch.int32, device="cuda")
    w_tables = dict(count=count, keys=keys, key_index=kidx)
    wg = (WG.WgBatch(inp=raw, out=w_msg, status=w_st[0], receiver=t32(spi_h), counter=seq, lens=d_ilen, max_len=HI,
                     in_off=d_raw_off, out_off=d_wmsg_off, **w_tables),
          WG.WgBatch(inp=w_msg, out=w_back, status=w_st[1], counter_out=w_ctr_out, inner_len=w_ilen_out, lens=t32(wmlen),
                     max_len=int(wmlen.max()), in_off=d_wmsg_off, out_off=d_raw_off, **w_tables))

    # the AEAD alone, as before: trailers, nonces and ADs built on the host side of the call (none is timed)
    be = lambda a: a.astype(">u4").view(np.uint8).reshape(count, 4)  # noqa: E731
    nonces = np.zeros((count, 12), dtype=np.uint8)
    nonces[:, :4] = salts_h.reshape(SAS, 4)[kidx_h]
    nonces[:, 4:] = seq_h.astype(">u8").view(np.uint8).reshape(count, 8)
    ads = np.concatenate([be(spi_h[kidx_h]), be((seq_h >> np.uint64(32)).astype(u32)), be(seq_h.astype(u32))], axis=1)
    r_ct_off = cum(plen + u32(16))
    r_ct_bytes = int(r_ct_off[-1] + plen[-1] + 16)
    r_pt = raw.clone()
    end = d_raw_off + t64(ilen.astype(np.uint64))
    d_pad = t64(pad.astype(np.uint64))
    for j in range(ALIGN - 1):
        at = end[d_pad > j] + j
        r_pt[at] = j + 1
    r_pt[end + d_pad] = d_pad.to(torch.uint8)
    r_pt[end + d_pad + 1] = nh
    r_ct, r_back = empty(r_ct_bytes), empty(raw_bytes)
    r_st = torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = empty(B.workspace_size(count))
    common = dict(count=count, keys=keys.view(SAS, 32), key_index=kidx, tls=False, rfc8439=True,
                  nonces=t8(nonces.tobytes()), ads=t8(np.ascontiguousarray(ads).tobytes()), ad_len=12, ad_stride=12, workspace=ws)
    d_ct_off, d_plen = t64(r_ct_off), t32(plen)
    rfc = (B.Batch(inp=r_pt, out=r_ct, lens=d_plen, max_len=int(plen.max()), in_off=d_raw_off, out_off=d_ct_off, **common),
           B.Batch(inp=r_ct, out=r_back, lens=t32(plen + u32(16)), max_len=int(plen.max()) + 16, in_off=d_ct_off,
                   out_off=d_raw_off, status=r_st, **common))

    raw_host = raw.cpu().numpy()

    def packet(i, buf):  # (key, salt, spi, seq, payload, next header, top, the packet in buf) of packet i
        k, o, q = int(kidx_h[i]), int(raw_off[i]), int(msg_off[i])
        return (keys_h[32 * k:32 * k + 32], salts_h[4 * k:4 * k + 4].tobytes(), int(spi_h[k]), int(seq_h[i]),
                raw_host[o:o + int(ilen[i])].tobytes(), int(nh_h[i]), int(top_h[k]), buf[q:q + int(mlen[i])].cpu().numpy().tobytes())

    return dict(count=count, payload=int(plen.sum()), wg_payload=int(wlen.sum()), esp=esp, espp=espp, wg=wg, rfc=rfc, raw=raw,
                msg=msg, back=back, place=place, start=start, sealed=sealed, st=st, w_st=w_st, r_st=r_st, seq=seq, seq_out=seq_out,
                ilen=d_ilen, plen=t64(plen.astype(np.uint64)), plen_out=plen_out, nh=nh, nh_out=nh_out, w_ctr_out=w_ctr_out,
                w_ilen_out=w_ilen_out, r_back=r_back, r_ct=r_ct, packet=packet, raw_off=d_raw_off, msg_off=d_msg_off,
                ct_off=d_ct_off, min_len=int(ilen.min()),
                desc=f"{count} payloads, lengths {LO}..{HI} (mean {ilen.mean():.0f} B, padded {plen.mean():.0f} B), "
                     f"{SAS} SAs, align {ALIGN}, ESN, window {WINDOW}")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import batch as B
    from suruga_amd import esp as ESP
    from suruga_amd import wg as WG

    # the in-place legs' start images: the payloads in their slots, and their sealed form
    w["place"].copy_(w["start"])
    ESP.seal_esp(w["espp"][0])
    w["sealed"].copy_(w["place"])
    legs = {"esp_seal": lambda: ESP.seal_esp(w["esp"][0]), "esp_open": lambda: ESP.open_esp(w["esp"][1]),
            "esp_inplace_seal": (lambda: w["place"].copy_(w["start"]), lambda: ESP.seal_esp(w["espp"][0])),
            "esp_inplace_open": (lambda: w["place"].copy_(w["sealed"]), lambda: ESP.open_esp(w["espp"][1])),
            "wg_seal": lambda: WG.seal_wg(w["wg"][0]), "wg_open": lambda: WG.open_wg(w["wg"][1]),
            "rfc_seal": lambda: B.seal(w["rfc"][0]), "rfc_open": lambda: B.open_(w["rfc"][1])}
    # one pass in order first, so that every open leg has its input
    for name in ("esp_seal", "esp_open", "wg_seal", "wg_open", "rfc_seal", "rfc_open"):
        legs[name]()
    times = ab_legs.timed_legs(legs, reps, warmup)
    w["place"].copy_(w["sealed"])  # whichever in-place leg ran last: leave the opened image behind
    ESP.open_esp(w["espp"][1])
    torch.cuda.synchronize()
    for s in (w["st"], w["w_st"], w["r_st"]):
        assert int(s.sum().item()) == 0, "status"
    for k in (0, 1):
        assert torch.equal(w["seq_out"][k], w["seq"]), "sequence numbers"
        assert torch.equal(w["plen_out"][k], w["ilen"]) and torch.equal(w["nh_out"][k], w["nh"]), "payload lengths and next headers"
    assert torch.equal(w["w_ctr_out"], w["seq"]) and torch.equal(w["w_ilen_out"], w["ilen"]), "WireGuard counters and lengths"
    # the round trip -- every packet's first, second and (of the shortest) last payload byte -- and the two
    # constructions agree on ciphertext and ICV
    ro, mo, co, P = w["raw_off"], w["msg_off"], w["ct_off"], w["plen"]
    for d in (0, 1, w["min_len"] - 1):
        want = w["raw"][ro + d]
        assert torch.equal(w["back"][ro + d], want) and torch.equal(w["place"][mo + 16 + d], want), "round trip"
        assert torch.equal(w["r_back"][ro + d], want), "round trip (rfc)"
    for d in (0, 7, 1000):
        assert torch.equal(w["msg"][mo + 16 + d], w["r_ct"][co + d]) and torch.equal(w["sealed"][mo + 16 + d], w["r_ct"][co + d])
    for d in (-1, 0, 15):  # the trailer's last byte and the ICV's ends
        assert torch.equal(w["msg"][mo + 16 + P + d], w["r_ct"][co + P + d]), "trailer and ICV"
        assert torch.equal(w["sealed"][mo + 16 + P + d], w["r_ct"][co + P + d]), "trailer and ICV (in place)"
    out = {"batch": w["desc"], "payload_bytes": w["payload"], "wg_payload_bytes": w["wg_payload"]}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["wg_payload"] if name.startswith("wg_") else w["payload"])
        out[name]["mpps"] = round(w["count"] / (out[name]["ms"] * 1e-3) / 1e6, 1)
    for d in ("seal", "open"):
        for a in ("esp", "esp_inplace"):
            for b in ("wg", "rfc"):
                out[f"{a}_vs_{b}_{d}"] = round(out[f"{a}_{d}"]["ms"] / out[f"{b}_{d}"]["ms"], 4)
    out["rfc_legs"] = "AEAD only; the host's nonce, AD and trailer work is not in their number"
    out["not_measured"] = ("the host work the rfc legs leave out; align above 4 (more bytes made on seal, more read back on "
                           "open); ESN off (an 8-byte AD: the same one block); other length mixes; more than one stream")
    return out


def check(w: dict) -> dict:
    """A sample of packets, of both seal legs, against tests/esp_ref.py, and back."""
    import esp_ref as E

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        for buf in (w["msg"], w["sealed"]):
            key, salt, spi, seq, payload, nh, top, got = w["packet"](i, buf)
            assert got == E.protect(key, salt, spi, seq, payload, nh, align=ALIGN, esn=True), f"packet {i} differs from the reference"
            pt = payload + E.trailer(E.pad_len(len(payload), ALIGN), nh)
            assert E.unprotect(key, salt, spi, got, esn=True, top=top, window=WINDOW) == (0, pt, seq, len(payload), nh)
    return {"packets_checked": len(idx), "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--packets", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "esp_bench.json"), help="where the JSON goes ('' : nowhere)")
    args = ap.parse_args()
    assert args.reps >= 25 or args.out == "", "a recorded run takes at least 25 rounds"

    res, bus = ab_legs.prelude("esp_bench", args.reps, args.warmup)
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
