"""The decode queue's typed items on the CPU: the position map its decoders store through
(smallz4_amd/csrc/sz4_typed_map.h) against the host model of the byte-plane merge (smallz4_amd/planes.py).
tests/cpp/typed_map_check.cpp includes the header, checks for every width and every length 0..71 and
4093..4100 that the map is a permutation, and prints it; here every byte of a random split is put where the
map says, and the result must be planes.merge of that split.  The program is compiled as host code with the
address and undefined-behaviour sanitizers and runs stand-alone: no GPU, nothing loaded into Python."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from smallz4_amd import planes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(0, 72)) + list(range(4093, 4101))


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{(E, n): [address of position x]} as the program printed it."""
    if shutil.which("hipcc") is None:
        pytest.skip("no hipcc")
    exe = tmp_path_factory.mktemp("typed_map") / "typed_map_check"
    subprocess.run(["hipcc", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined",
                    os.path.join(ROOT, "tests", "cpp", "typed_map_check.cpp"), "-o", str(exe)], check=True)
    env = dict(os.environ, UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    print(r.stderr)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().endswith("typed_map_check ok")
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    out = {}
    for line in r.stdout.splitlines()[:-1]:
        head, _, rest = line.partition(":")
        E, n = (int(v) for v in head.split())
        out[(E, n)] = [int(v) for v in rest.split()]
    return out


def test_every_case_is_a_permutation(maps):
    assert set(maps) == {(E, n) for E in planes.WIDTHS for n in LENGTHS}
    for (E, n), addr in maps.items():
        assert sorted(addr) == list(range(n)), (E, n)


def test_storing_through_the_map_is_the_merge(maps):
    rng = np.random.default_rng(81)
    for (E, n), addr in sorted(maps.items()):
        split = rng.integers(0, 256, n, dtype=np.uint8)
        merged = np.zeros(n, dtype=np.uint8)
        merged[np.asarray(addr, dtype=np.int64)] = split
        assert merged.tobytes() == planes.merge(split.tobytes(), E), (E, n)
        # and the other way round: the map reads the item the way split() lays it out
        assert planes.split(merged.tobytes(), E) == split.tobytes(), (E, n)


def test_width_one_and_short_items_are_the_identity(maps):
    for (E, n), addr in maps.items():
        if E == 1 or n < E:
            assert addr == list(range(n)), (E, n)
