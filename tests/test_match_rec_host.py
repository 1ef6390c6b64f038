"""The token walk's 8-byte match record and the encoded size of a sequence (smallz4_amd/csrc/sz4_match_rec.h)
on the CPU: tests/cpp/match_rec_check.cpp packs and unpacks positions, lengths and distances at the edges of
their fields, and compares token_bytes with a naive LZ4 sequence encoder that counts the bytes it writes, over
literal counts 0..600 x match lengths 4..600 and around every length-code edge (14, 15, 16, 15 + 255 k +- 1),
with and without the closing-run flag.  The program is compiled as host code with the address and
undefined-behaviour sanitizers, includes the header alone and runs stand-alone: no GPU, nothing loaded into
Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc")
def test_match_rec_under_sanitizers(tmp_path):
    exe = tmp_path / "match_rec_check"
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "cpp", "match_rec_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stdout)
    print(r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("match_rec_check ok")
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
