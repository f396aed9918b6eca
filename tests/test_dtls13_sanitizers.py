"""The host-only code of the DTLS 1.3 record batch (the argument rules of
sg_seal_batch_dtls13 / sg_open_batch_dtls13, sg_dtls13_header_len, sg_dtls13_inner_len,
sg_dtls13_record_len, and the sequence number's reconstruction the kernel shares with them)
under AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/test_dtls13_san.cpp, a
stand-alone program with its own main, built with g++ -fsanitize=address,undefined from
sg_dtls13_host.cpp alone and run directly.

CPU only: no GPU, no HIP header, nothing loaded into Python."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1",
           "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_dtls13_host_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "test_dtls13_san"
    csrc = ROOT / "suruga_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", str(exe),
           str(ROOT / "tests" / "cpp" / "test_dtls13_san.cpp"), str(csrc / "sg_dtls13_host.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "dtls13 sanitizer checks passed" in r.stdout
