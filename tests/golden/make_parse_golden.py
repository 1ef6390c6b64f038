"""Regenerate tests/golden/parse_cases.json: the REFERENCE's own frames for the constructed parse cases.

For every base case of tests/golden/parsecases.py and every level it is meant for, this runs the reference
(oracle/_ref/libsmallz4_ref.so, compiled in place by oracle/Makefile) and records the input's length and
SHA-256 and the frame's length and SHA-256 -- no frame bytes.  Every case is one block (the reference cuts at
4 MiB), so the frame is the smallz4 header, the block and the end mark.  Sweep variants get no fixture.

    python tests/golden/make_parse_golden.py [-j 8]
"""
from __future__ import annotations

import argparse
import hashlib
import json
import os
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import parsecases  # noqa: E402
from oracle import pyoracle  # noqa: E402


def sha(b: bytes) -> str:
    return hashlib.sha256(b).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    if not pyoracle.ref_available():
        sys.exit("oracle/_ref/libsmallz4_ref.so missing: run `make -C oracle` with the reference present")
    cases = parsecases.base_cases()
    jobs = [(c, chain) for c in cases for chain in c.levels]
    with ThreadPoolExecutor(max_workers=a.j) as ex:  # ctypes releases the GIL
        frames = list(ex.map(lambda j: pyoracle.ref_lz4(j[0].data, j[1]), jobs))
    out = {}
    for (c, chain), frame in zip(jobs, frames):
        e = out.setdefault(c.name, {"name": c.name, "family": c.family, "input_len": len(c.data),
                                    "input_sha256": sha(c.data), "levels": {}})
        e["levels"][str(chain)] = {"frame_len": len(frame), "frame_sha256": sha(frame)}
    with open(os.path.join(HERE, "parse_cases.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_parse_golden.py",
                   "reference": "gbonneau-hardent/smallz4 @ 2025-01-17, smallz4::lz4 via oracle/_ref",
                   "cases": [out[c.name] for c in cases]}, f, indent=1)
    print(f"{len(cases)} cases, {len(jobs)} frames")


if __name__ == "__main__":
    main()
