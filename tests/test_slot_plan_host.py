"""The slot plan of a sized compress queue (smallz4_amd/csrc/sz4_slot_plan.h, Plan::build_slots) on the CPU:
tests/cpp/slot_plan_check.cpp derives every slot's entries for sizes that sweep the plan's edges and compares
them with the planner's own one-block plans moved to the slot's offsets; what a size does not need must be
inert, and nothing may exceed what the capacity reserved.  The program is compiled as host code with the
address and undefined-behaviour sanitizers, links the planner alone and runs stand-alone: no GPU, nothing
loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_slot_plan_under_sanitizers(tmp_path):
    exe = tmp_path / "slot_plan_check"
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "cpp", "slot_plan_check.cpp"),
                    os.path.join(ROOT, "smallz4_amd", "csrc", "sz4_plan.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    env.pop("SZ4_DP_SIZE", None)  # the planner's tuning knob does not apply to slots: the reference plans must not use it
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("slot_plan_check ok")
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
