"""The device memory accounting (smallz4_amd/csrc/sz4_mem.h: Budget, DevBuf) on the CPU: tests/cpp/mem_check.cpp
drives seeded random sequences of reserve / release / shed / detach / next call over a dozen buffers, with and
without a limit, with and without a capacity of the (stand-in) device, and with the failure hooks
SZ4_TEST_ALLOC_CAP / SZ4_TEST_FAIL_RESERVE set, and compares every field with a plain model after every step.
tests/cpp/fakehip stands in for the HIP header (malloc with a settable capacity), so the program is host code
alone: compiled with the address and undefined-behaviour sanitizers, no HIP library linked, run stand-alone,
nothing loaded into Python.  LeakSanitizer reports at exit what a lost buffer would leave behind."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_accounting_under_sanitizers(tmp_path):
    exe = tmp_path / "mem_check"
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "tests", "cpp", "fakehip"),  # first: its <hip/hip_runtime.h> is the one found
                    "-I", os.path.join(ROOT, "smallz4_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "mem_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("mem_check ok")
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
