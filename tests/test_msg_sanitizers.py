"""The long-message plan (suruga_amd/csrc/sg_msg_plan.cpp: host only, no HIP)
built with g++ -fsanitize=address,undefined into the stand-alone program
tests/cpp/test_msg_plan_san.cpp, which runs the sweep of tests/test_msg_plan.py.
Built and run as tests/test_sanitizers.py does its host program: its own
``main``, nothing preloaded.  CPU only."""
from __future__ import annotations

import os
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = {"ASAN_OPTIONS": "detect_leaks=0:abort_on_error=1:halt_on_error=1",
           "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"}


def test_msg_plan_under_asan_ubsan(tmp_path):
    exe = tmp_path / "test_msg_plan_san"
    cmd = ["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", *SAN, "-o", str(exe),
           str(ROOT / "tests" / "cpp" / "test_msg_plan_san.cpp"),
           str(ROOT / "suruga_amd" / "csrc" / "sg_msg_plan.cpp")]
    p = subprocess.run(cmd, capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600, env=dict(os.environ, **SAN_ENV))
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "msg plan sanitizer checks passed" in r.stdout
