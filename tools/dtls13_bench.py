#!/usr/bin/env python3
"""Rate of the DTLS 1.3 record batch (sg_seal_batch_dtls13 / sg_open_batch_dtls13) beside its
sibling kernel and beside the AEAD share a DTLS caller could get from the library before.
Prints one JSON line and writes it to profiles/dtls13_bench.json.

The batch: ``--records`` (default 2^20) contents of 256 connections, lengths uniform in
1,200..1,452 bytes (what tools/esp_bench.py draws), lying back to back at whatever address
that gives them; per-record types, no padding.  Four pairs of legs in one process:

* ``dtls_seal`` / ``dtls_open``: the DTLS calls with an 8-byte connection ID, a 16-bit
  sequence number and the length field (a 13-byte header) -- header, nonce, type byte, AEAD
  and the record number mask on seal; the header's checks, the unmasking, the sequence
  number's reconstruction, the tag and the strip on open, all on the device;
* ``dtls_min_seal`` / ``dtls_min_open``: the same with the minimal 2-byte header (no
  connection ID, an 8-bit sequence number, no length field).  With 4,096 records a
  connection and a window of 256 numbers, the sequence numbers of this pair repeat within a
  connection (base + rank mod 128): a timing input, not a sender's practice;
* ``quic_seal`` / ``quic_open``: ``sg_*_batch_quic`` over short-header packets (pn_off 9, a
  2-byte packet number: an 11-byte header) whose payloads are as long as the DTLS inner
  plaintexts -- the sibling kernel with the same mask work, which reads its header from the
  input and has nothing to make on seal and nothing to strip on open;
* ``rfc_seal`` / ``rfc_open``: ``sg_*_batch_rfc8439`` in explicit mode with the 13-byte header
  as AD over inner plaintexts whose type byte was set on the host, with nonces and ADs built
  on the host: what a DTLS caller had before.  It is the AEAD only: no header is written or
  checked, nothing is masked or unmasked, no sequence number rebuilt, nothing stripped, and
  the host's work is NOT in its number.

The legs alternate launch by launch, every round in another order (a seeded shuffle,
tools/ab_legs.py); each reports the median of ``--reps`` launches after ``--warmup`` from
HIP events, GiB/s of its own AEAD payload and ``spread`` = (max - min) / median.  The
``*_vs_*`` figures are a DTLS leg's time over the other leg's: figures to report beside the
spreads, not bounds -- nothing else in the library produces the DTLS legs' output.  A
sample of records is compared with tests/dtls13_ref.py, every byte; every record must open
with its 64-bit sequence number, content length and type and round-trip.

    python tools/dtls13_bench.py [--records 1048576] [--reps 25]
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

SEED = 0x64746c73
SAMPLE = 24
CONNS = 256
LO, HI = 1200, 1452
CID_LEN = 8
HDR, HDR_MIN = 1 + CID_LEN + 2 + 2, 2
Q_PN_OFF, Q_HDR = 9, 11
EPOCH = 3


def make(count: int):
    import numpy as np
    import torch

    from suruga_amd import batch as B
    from suruga_amd import dtls13 as DT
    from suruga_amd import quic as QU

    rng = np.random.default_rng(SEED)
    u32, u64 = np.uint32, np.uint64
    ilen = rng.integers(LO, HI + 1, size=count).astype(u32)  # content lengths
    inner = ilen + u32(1)                                     # ... and the AEAD's: content and type byte
    cum = lambda a: np.concatenate([[0], np.cumsum(a[:-1], dtype=u64)]).astype(u64)  # noqa: E731
    rlen, rlen_min, qraw_len = inner + u32(HDR + 16), inner + u32(HDR_MIN + 16), inner + u32(Q_HDR)
    raw_off, rec_off, rec_min_off, qraw_off, qprot_off, ct_off = (cum(a) for a in (inner, rlen, rlen_min, qraw_len,
                                                                                   qraw_len + u32(16), inner + u32(16)))
    total = lambda off, a: int(off[-1] + a[-1])  # noqa: E731
    kidx_h = rng.integers(0, CONNS, size=count).astype(u32)
    # a record's rank within its connection; the numbers of a connection run on from a base across a multiple of 2^16
    order = np.argsort(kidx_h, kind="stable")
    first = np.searchsorted(kidx_h[order], np.arange(CONNS))
    rank = np.empty(count, dtype=u64)
    rank[order] = np.arange(count, dtype=u64) - first[kidx_h[order]].astype(u64)
    base_h = (rng.integers(1, 2**30, size=CONNS).astype(u64) << u64(16)) - u64(1000)
    seq_h = base_h[kidx_h] + rank
    assert int(rank.max()) < 2**15 - 2
    expected_h = base_h + u64(int(rank.max()) // 2)
    seq_min_h = base_h[kidx_h] + rank % u64(128)
    expected_min_h = base_h + u64(64)
    type_h = rng.integers(1, 256, size=count, dtype=np.uint8)
    keys_h, ivs_h, sns_h = (rng.integers(0, 256, w * CONNS, dtype=np.uint8).tobytes() for w in (32, 12, 32))
    cids_h = rng.integers(0, 256, CID_LEN * CONNS, dtype=np.uint8)
    t8 = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda")  # noqa: E731
    t64 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to("cuda")  # noqa: E731
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to("cuda")  # noqa: E731
    empty = lambda n: torch.empty(n, dtype=torch.uint8, device="cuda")  # noqa: E731

    # the contents, each in a slot one byte longer; the byte behind a content is not its type
    raw_bytes = total(raw_off, inner)
    raw = empty(raw_bytes)
    B.fill_records(raw, 0, raw_bytes, 1, SEED)
    d_raw_off, d_rec_off, d_rec_min_off = t64(raw_off), t64(rec_off), t64(rec_min_off)
    keys, kidx, types = t8(keys_h), t32(kidx_h), t8(type_h.tobytes())
    d_ilen = t32(ilen)
    tables = dict(count=count, keys=keys, ivs=t8(ivs_h), sn_keys=t8(sns_h), key_index=kidx)
    st = torch.full((4, count), 0xFF, dtype=torch.uint8, device="cuda")
    seq_out = torch.zeros((2, count), dtype=torch.int64, device="cuda")
    clen_out = torch.zeros((2, count), dtype=torch.int32, device="cuda")
    ep_out = torch.zeros((2, count), dtype=torch.uint8, device="cuda")
    ty_out = torch.zeros((2, count), dtype=torch.uint8, device="cuda")
    rec, rec_min, back, back_min = empty(total(rec_off, rlen)), empty(total(rec_min_off, rlen_min)), empty(raw_bytes), empty(raw_bytes)
    seq, seq_min = t64(seq_h), t64(seq_min_h)

    def pair(k, out, off, lens, s, expected, plain, **form):
        outs = dict(seq_out=seq_out[k], epoch_out=ep_out[k], content_len=clen_out[k], type_out=ty_out[k])
        return (DT.Dtls13Batch(inp=raw, out=out, status=st[2 * k], seq=s, type=types, uniform_epoch=EPOCH, lens=d_ilen, max_len=HI,
                               in_off=d_raw_off, out_off=off, **form, **tables),
                DT.Dtls13Batch(inp=out, out=plain, status=st[2 * k + 1], expected=t64(expected), lens=t32(lens),
                               max_len=int(lens.max()), in_off=off, out_off=d_raw_off, cid_len=form.get("cid_len", 0), **outs,
                               **tables))

    dtls = pair(0, rec, d_rec_off, rlen, seq, expected_h, back, cids=t8(cids_h.tobytes()), cid_len=CID_LEN, seq16=True, length=True)
    dtls_min = pair(1, rec_min, d_rec_min_off, rlen_min, seq_min, expected_min_h, back_min)

    # the sibling: QUIC short-header packets with payloads of the inner plaintexts' lengths
    qraw_bytes, qprot_bytes = total(qraw_off, qraw_len), total(qprot_off, qraw_len + u32(16))
    qraw, qprot, qback = empty(qraw_bytes), empty(qprot_bytes), empty(qraw_bytes)
    B.fill_records(qraw, 0, qraw_bytes, 1, SEED + 1)
    d_qraw_off, d_qprot_off = t64(qraw_off), t64(qprot_off)
    qraw[d_qraw_off] = 0x41  # a short header with a 2-byte packet number
    q_st = torch.full((2, count), 0xFF, dtype=torch.uint8, device="cuda")
    q_pn_out = torch.zeros(count, dtype=torch.int64, device="cuda")
    q_tables = dict(count=count, keys=keys, ivs=tables["ivs"], hp_keys=tables["sn_keys"], key_index=kidx, uniform_pn_off=Q_PN_OFF)
    quic = (QU.QuicBatch(inp=qraw, out=qprot, status=q_st[0], pn=seq, lens=t32(qraw_len), max_len=int(qraw_len.max()),
                         in_off=d_qraw_off, out_off=d_qprot_off, **q_tables),
            QU.QuicBatch(inp=qprot, out=qback, status=q_st[1], pn=t64(expected_h[kidx_h]), pn_out=q_pn_out, lens=t32(qraw_len + u32(16)),
                         max_len=int(qraw_len.max()) + 16, in_off=d_qprot_off, out_off=d_qraw_off, **q_tables))

    # the AEAD alone, as before: type bytes, nonces and ADs built on the host side of the call (none is timed)
    nonces = np.frombuffer(ivs_h, dtype=np.uint8).reshape(CONNS, 12)[kidx_h].copy()
    nonces[:, 4:] ^= seq_h.astype(">u8").view(np.uint8).reshape(count, 8)
    ads = np.empty((count, HDR), dtype=np.uint8)
    ads[:, 0] = 0x20 | 0x10 | 0x08 | 0x04 | EPOCH
    ads[:, 1:1 + CID_LEN] = cids_h.reshape(CONNS, CID_LEN)[kidx_h]
    ads[:, 1 + CID_LEN:3 + CID_LEN] = seq_h.astype(">u8").view(np.uint8).reshape(count, 8)[:, 6:]
    ads[:, 3 + CID_LEN:] = (inner + u32(16)).astype(">u2").view(np.uint8).reshape(count, 2)
    r_pt = raw.clone()
    r_pt[d_raw_off + t64(ilen.astype(u64))] = types
    r_ct, r_back = empty(total(ct_off, inner + u32(16))), empty(raw_bytes)
    r_st = torch.full((count,), 0xFF, dtype=torch.uint8, device="cuda")
    ws = empty(B.workspace_size(count))
    common = dict(count=count, keys=keys.view(CONNS, 32), key_index=kidx, tls=False, rfc8439=True, nonces=t8(nonces.tobytes()),
                  ads=t8(ads.tobytes()), ad_len=HDR, ad_stride=HDR, workspace=ws)
    d_ct_off = t64(ct_off)
    rfc = (B.Batch(inp=r_pt, out=r_ct, lens=t32(inner), max_len=int(inner.max()), in_off=d_raw_off, out_off=d_ct_off, **common),
           B.Batch(inp=r_ct, out=r_back, lens=t32(inner + u32(16)), max_len=int(inner.max()) + 16, in_off=d_ct_off,
                   out_off=d_raw_off, status=r_st, **common))

    raw_host = raw.cpu().numpy()

    def record(i, which):  # (key, iv, sn_key, cid, seq, expected, content, type, the record) of record i in either form
        k, o = int(kidx_h[i]), int(raw_off[i])
        buf, off, lens, s, e = ((rec, rec_off, rlen, seq_h, expected_h) if which == 0
                                else (rec_min, rec_min_off, rlen_min, seq_min_h, expected_min_h))
        q = int(off[i])
        return (keys_h[32 * k:32 * k + 32], ivs_h[12 * k:12 * k + 12], sns_h[32 * k:32 * k + 32],
                cids_h[CID_LEN * k:CID_LEN * (k + 1)].tobytes() if which == 0 else b"", int(s[i]), int(e[k]),
                raw_host[o:o + int(ilen[i])].tobytes(), int(type_h[i]), buf[q:q + int(lens[i])].cpu().numpy().tobytes())

    return dict(count=count, payload=int(inner.sum(dtype=np.uint64)), dtls=dtls, dtls_min=dtls_min, quic=quic, rfc=rfc, raw=raw,
                rec=rec, rec_min=rec_min, back=back, back_min=back_min, st=st, q_st=q_st, r_st=r_st, seq=seq, seq_min=seq_min,
                seq_out=seq_out, clen_out=clen_out, ep_out=ep_out, ty_out=ty_out, ilen=d_ilen, types=types, q_pn_out=q_pn_out,
                r_back=r_back, r_ct=r_ct, record=record, raw_off=d_raw_off, rec_off=d_rec_off, ct_off=d_ct_off,
                inner=t64(inner.astype(u64)), min_len=int(ilen.min()),
                desc=f"{count} contents, lengths {LO}..{HI} (mean {ilen.mean():.0f} B), {CONNS} connections, no padding; "
                     f"header {HDR} B (cid_len {CID_LEN}, 16-bit sequence number, length) and {HDR_MIN} B")


def run(w: dict, reps: int, warmup: int) -> dict:
    import torch

    from suruga_amd import batch as B
    from suruga_amd import dtls13 as DT
    from suruga_amd import quic as QU

    legs = {"dtls_seal": lambda: DT.seal_dtls13(w["dtls"][0]), "dtls_open": lambda: DT.open_dtls13(w["dtls"][1]),
            "dtls_min_seal": lambda: DT.seal_dtls13(w["dtls_min"][0]), "dtls_min_open": lambda: DT.open_dtls13(w["dtls_min"][1]),
            "quic_seal": lambda: QU.seal_quic(w["quic"][0]), "quic_open": lambda: QU.open_quic(w["quic"][1]),
            "rfc_seal": lambda: B.seal(w["rfc"][0]), "rfc_open": lambda: B.open_(w["rfc"][1])}
    for name in legs:  # one pass in order first, so that every open leg has its input
        legs[name]()
    times = ab_legs.timed_legs(legs, reps, warmup)
    torch.cuda.synchronize()
    for s in (w["st"], w["q_st"], w["r_st"]):
        assert int(s.sum().item()) == 0, "status"
    assert torch.equal(w["seq_out"][0], w["seq"]) and torch.equal(w["seq_out"][1], w["seq_min"]), "sequence numbers"
    assert torch.equal(w["q_pn_out"], w["seq"]), "QUIC packet numbers"
    for k in (0, 1):
        assert torch.equal(w["clen_out"][k], w["ilen"]) and torch.equal(w["ty_out"][k], w["types"]), "content lengths and types"
        assert int((w["ep_out"][k] != EPOCH).sum().item()) == 0, "epoch bits"
    # the round trip -- every record's first, second and (of the shortest) last content byte -- and the two
    # constructions agree on ciphertext and tag
    ro, mo, co, P = w["raw_off"], w["rec_off"], w["ct_off"], w["inner"]
    for d in (0, 1, w["min_len"] - 1):
        want = w["raw"][ro + d]
        assert torch.equal(w["back"][ro + d], want) and torch.equal(w["back_min"][ro + d], want), "round trip"
        assert torch.equal(w["r_back"][ro + d], want), "round trip (rfc)"
    for d in (0, 7, 1000):
        assert torch.equal(w["rec"][mo + HDR + d], w["r_ct"][co + d]), "ciphertext"
    for d in (-1, 0, 15):  # the type byte's ciphertext and the tag's ends
        assert torch.equal(w["rec"][mo + HDR + P + d], w["r_ct"][co + P + d]), "type byte and tag"
    out = {"batch": w["desc"], "payload_bytes": w["payload"]}
    for name, ms in times.items():
        out[name] = ab_legs.summary(ms, w["payload"])
        out[name]["mpps"] = round(w["count"] / (out[name]["ms"] * 1e-3) / 1e6, 1)
    for d in ("seal", "open"):
        for a in ("dtls", "dtls_min"):
            for b in ("quic", "rfc"):
                out[f"{a}_vs_{b}_{d}"] = round(out[f"{a}_{d}"]["ms"] / out[f"{b}_{d}"]["ms"], 4)
    out["rfc_legs"] = "AEAD only; the host's type byte, nonce, AD, mask and strip work is not in their number"
    out["not_measured"] = ("the host work the rfc legs leave out; pad_to above 1 (bytes made on seal, more rounds of the strip on "
                           "open); epoch rows; a long connection ID; records above 2 KiB (16 lanes); other length mixes; more "
                           "than one stream")
    return out


def check(w: dict) -> dict:
    """A sample of records, of both header forms, against tests/dtls13_ref.py, and back."""
    import dtls13_ref as D

    idx = ab_legs.sample_indices(w["count"], SAMPLE)
    t0 = time.perf_counter()
    for i in idx:
        for which in (0, 1):
            key, iv, sn, cid, seq, expected, content, ctype, got = w["record"](i, which)
            want = D.protect(key, iv, sn, seq, content, ctype, epoch=EPOCH, cid=cid, seq16=which == 0, length=which == 0)
            assert got == want, f"record {i} (form {which}) differs from the reference"
            opened = D.unprotect(lambda ee: (key, iv, sn, expected), got, len(cid))
            assert opened == (0, content + bytes([ctype]), seq, EPOCH, len(content), ctype)
    return {"records_checked": 2 * len(idx), "check_s": round(time.perf_counter() - t0, 2)}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--records", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "dtls13_bench.json"), help="where the JSON goes ('' : nowhere)")
    args = ap.parse_args()
    assert args.reps >= 25 or args.out == "", "a recorded run takes at least 25 rounds"

    res, bus = ab_legs.prelude("dtls13_bench", args.reps, args.warmup)
    w = make(args.records)
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
