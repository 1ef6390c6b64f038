"""Regenerate tests/golden/emit_records.json: the oracle's frames for the inputs of tests/test_emit_records.py
that the oracle is too slow to redo inside a GPU test (its chain walk is quadratic in a run or a short
period: 5 to 40 s per input).  The frames themselves are recorded -- they are a few KB at most -- built as
tests/test_gpu.py's expected_frame builds them (header, oz_block of every block, end mark), with the SHA-256 of
the input, so a change of an input is caught.

    python tests/golden/make_emit_records_golden.py
"""
from __future__ import annotations

import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_emit_records as T  # noqa: E402  (the inputs and expected_frame)


def main():
    cases = []
    for name, (make, block_sizes, chains) in sorted(T.RECORDED.items()):
        data = make()
        for bs in block_sizes:
            for chain in chains:
                frame = T.expected_frame(data, bs, chain)
                cases.append({"name": name, "input_len": len(data), "input_sha256": hashlib.sha256(data).hexdigest(),
                              "block_size": bs, "max_chain": chain, "frame_hex": frame.hex()})
                print(f"{name:12s} bs {bs:8d} chain {chain:5d}: {len(frame)} B", flush=True)
    with open(os.path.join(HERE, "emit_records.json"), "w") as f:
        json.dump({"generator": "tests/golden/make_emit_records_golden.py", "oracle": "oracle/pyoracle.py oz_block",
                   "cases": cases}, f, indent=1)


if __name__ == "__main__":
    main()
