"""The record layer's pipeline switches under the RFC 7905 / TLS 1.3 calls (GPU).

sg_record.cpp reads its pipeline switches once per process, so each form runs a
selection of tests/test_gpu_record13.py in a child process of its own, as
tests/test_gpu_record_variants.py does for the draft calls:

* SG_RECORD_KD2H=1: the zero-copy TLS 1.3 read's gather kernel writes the caller's
  registered `out` itself, at the offset the cursor chain hands it (the write's
  frame kernel builds the wire in `wire`);
* SG_RECORD_SDMA=1: staged calls through the copy-engine pipeline, where the gather
  fills a device chunk buffer and exactly the delivered bytes are copied out;
* SG_RECORD_SLOTS=2: the shallowest pipeline.

SG_RECORD13_GATHER itself has a setter, which the selected tests use for both values;
that the environment gives its initial value is the last test here.

The selection: full records across the chunk seam at two `out` alignments, a
failing record of each kind as the last of chunk 0, and the failure's plaintext
staying out of `out`."""
from __future__ import annotations

import os
import subprocess
import sys
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent

VARIANTS = {
    "kd2h": {"SG_RECORD_KD2H": "1"},
    "sdma": {"SG_RECORD_SDMA": "1"},
    "shallow": {"SG_RECORD_SLOTS": "2"},
}
SELECT = "full_records_across or 255 or failure_leaves"


@pytest.mark.parametrize("name", sorted(VARIANTS))
def test_record13_pipeline_variant(gpu, name):
    env = dict(os.environ, **VARIANTS[name])
    args = [sys.executable, "-u", "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
            "tests/test_gpu_record13.py", "-k", SELECT]
    p = subprocess.run(args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=200)
    tail = (p.stdout + p.stderr)[-3000:]
    assert p.returncode == 0, tail
    assert " passed" in p.stdout and "skipped" not in p.stdout.splitlines()[-1], tail


def test_gather_switch_reads_the_environment(gpu):
    code = ("from suruga_amd import _native as N; lib = N.load(); a = lib.sg_set_record13_gather(-1); "
            "b = lib.sg_set_record13_gather(1 - a); print(a, b, lib.sg_set_record13_gather(-1))")
    for value, want in (("1", "1 1 0"), ("0", "0 0 1"), (None, "0 0 1")):
        env = {k: v for k, v in os.environ.items() if k != "SG_RECORD13_GATHER"}
        if value is not None:
            env["SG_RECORD13_GATHER"] = value
        p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0 and p.stdout.split("\n")[-2].strip() == want, (value, p.stdout, p.stderr[-1000:])
