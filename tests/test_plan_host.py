"""The block planner (smallz4_amd/csrc/sz4_plan.cpp) on the CPU: tests/cpp/plan_check.cpp builds uniform,
stream and ragged plans and checks them against values written out by hand from the definitions, and
the one-entry cache against its key.  The program is compiled as host code with the address and
undefined-behaviour sanitizers, links the planner alone and runs stand-alone: no GPU, nothing loaded
into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_planner_under_sanitizers(tmp_path):
    exe = tmp_path / "plan_check"
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "cpp", "plan_check.cpp"),
                    os.path.join(ROOT, "smallz4_amd", "csrc", "sz4_plan.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("SZ4_DP_SIZE", None)  # the planner's tuning knob would change the expected parse segments
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("plan_check ok")
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
