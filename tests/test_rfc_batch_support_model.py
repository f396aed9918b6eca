"""The host side of tests/rfc_batch_support.py without a GPU: RfcCase's TLS records
are the records OpenSSL sealed (tests/golden/rfc7905_records.json), its explicit
mode takes 12 bytes of nonce per record, and the forger reaches its targets."""
from __future__ import annotations

import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

import rfc8439_ref as R
import rfc_batch_support as S
from gpu_support import slots

DOC = json.loads((Path(__file__).resolve().parent / "golden" / "rfc7905_records.json").read_text())


def test_tls_case_gives_the_openssl_records():
    """One listed batch of every fixture record, two keys' worth of IVs under one key."""
    cases = DOC["cases"]
    key = bytes.fromhex(DOC["key"])
    lens = np.array([c["n"] for c in cases])
    in_off, out_off, pt_bytes, _ = slots(lens, 16)
    pt = bytearray(max(pt_bytes, 1))
    for c, o in zip(cases, in_off):
        pt[int(o):int(o) + c["n"]] = R.data(c["n"], b"rfc7905 pt %d" % c["n"])
    case = S.RfcCase(lens, bytes(pt), key + key, in_off=in_off, out_off=out_off,
                     kidx=np.array([c["iv"] for c in cases], dtype=np.uint32),
                     seqs=np.array([c["seq"] for c in cases], dtype=np.uint64),
                     ivs_h=b"".join(bytes.fromhex(x) for x in DOC["ivs"]), content_type=DOC["header"][0],
                     version=tuple(DOC["header"][1:]))
    for i, c in enumerate(cases):
        nonce, ad = case.nonce_ad(S.REF, i)
        assert (nonce.hex(), ad.hex()) == (c["nonce"], c["ad"])
        sealed = case.expected(S.REF, i)
        assert hashlib.sha256(sealed[:-16]).hexdigest() == c["ct_sha256"] and sealed[-16:].hex() == c["tag"], i


def test_explicit_case_reads_twelve_nonce_bytes_per_record():
    case = S.listed_case((5, 0, 40), mode=13, kidx=np.array([2, 0, 1], dtype=np.uint32), tag="model")
    assert len(case.nonces_h) == 36 and len(case.ads_h) == 39
    for i in range(3):
        nonce, ad = case.nonce_ad(S.REF, i)
        assert nonce == case.nonces_h[12 * i:12 * i + 12] and ad == case.ads_h[13 * i:13 * i + 13]
        assert case.expected(S.REF, i) == R.seal(S.KEYS3[32 * case.key_slot(i):][:32], nonce, case.pt(i), ad)
        rc, back = R.open(case.key(i), nonce, case.expected(S.REF, i), ad)
        assert rc == 0 and back == case.pt(i)
        assert R.open(case.key(i), nonce, case.expected(S.REF, i), ad + b"\0")[0] == 1  # the padding forgery


@pytest.mark.parametrize("name", list(S.ACC_TARGETS))
@pytest.mark.parametrize("n", [4096, 16384])
def test_forger_reaches_the_accumulator(name, n):
    key, nonce, ad = S.KEYS3[:32], S.rnd(12, f"model nonce {name}"), S.rnd(13, "model ad")
    ct, tries = S.forge_ct(key, nonce, ad, n, S.ACC_TARGETS[name], f"model {name} {n}")
    assert tries <= 200 and len(ct) == n
    h = S.accumulator(key, nonce, ad, ct)
    assert h == S.ACC_TARGETS[name] % S.P
    _, s16 = R.poly_key(key, nonce)
    want = ((h + int.from_bytes(s16, "little")) % (1 << 128)).to_bytes(16, "little")
    assert R.tag_of(key, nonce, ad, ct) == want
