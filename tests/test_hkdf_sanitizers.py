"""The host HKDF calls (sg_hkdf_extract, sg_hkdf_expand_label, sg_tls13_traffic_keys)
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/test_hkdf_san.cpp, a
stand-alone program with its own main (the length bounds and one past each, output
buffers of exactly out_len bytes, tables of exactly `count` rows on several threads),
built with g++ -fsanitize=address,undefined from sg_keysched.cpp alone and run directly.

CPU only: no GPU, no HIP header, nothing loaded into Python."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1",
           "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_hkdf_under_asan_ubsan(tmp_path):
    exe = tmp_path / "test_hkdf_san"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread", *SAN, "-o", str(exe),
           str(ROOT / "tests" / "cpp" / "test_hkdf_san.cpp"), str(ROOT / "suruga_amd" / "csrc" / "sg_keysched.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "hkdf sanitizer checks passed" in r.stdout
