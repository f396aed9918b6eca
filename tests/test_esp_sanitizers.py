"""The host-only code of the IPsec ESP batch (the argument rules of sg_seal_batch_esp /
sg_open_batch_esp, sg_esp_padded_len, sg_esp_packet_len, sg_esp_seq_hi) under
AddressSanitizer and UndefinedBehaviorSanitizer: tests/cpp/test_esp_san.cpp, a stand-alone
program with its own main, built with g++ -fsanitize=address,undefined from
sg_esp_host.cpp alone and run directly.

CPU only: no GPU, no HIP header, nothing loaded into Python."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=1:halt_on_error=1",
           "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_esp_host_code_under_asan_ubsan(tmp_path):
    exe = tmp_path / "test_esp_san"
    csrc = ROOT / "suruga_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *SAN, "-o", str(exe),
           str(ROOT / "tests" / "cpp" / "test_esp_san.cpp"), str(csrc / "sg_esp_host.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "esp sanitizer checks passed" in r.stdout
