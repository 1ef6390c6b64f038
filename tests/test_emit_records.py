"""The token walk's match records and the frame writer that reads them (k_walk .. k_write_seg in
smallz4_amd/csrc/sz4_kernels.hip): inputs built for the places where a record, a literal run derived from the
record before it, or a sub-segment's slots can go wrong.  Every case compares the GPU frame byte for byte with
the oracle's, built as tests/test_gpu.py builds it, at chains 65535 (optimal parse), 5 (lazy) and 1 (greedy)
unless the case says otherwise.  Run with -m gpu on an MI355X."""
import hashlib
import json
import os

import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x70, 0xDF])
CHAINS = (65535, 5, 1)


def expected_frame(data, bs, chain):
    return HDR + b"".join(pyoracle.oz_block(data[o:o + bs], chain) for o in range(0, len(data), bs)) + b"\0\0\0\0"


def rnd(n, seed):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def check(compressor, data, bs, chains=CHAINS):
    for chain in chains:
        got = compressor.compress_blocks(data, bs, chain)
        want = expected_frame(data, bs, chain)
        assert got == want, (len(data), bs, chain, len(got), len(want))


# Inputs on which the oracle needs 5 to 40 s (its chain walk is quadratic in a run or a short period): its frames,
# a few KB at most, are recorded in tests/golden/emit_records.json by tests/golden/make_emit_records_golden.py
# (name: input, block sizes, chains)
RECORDED = {
    "zeros70000": (lambda: bytes(70000), (65536,), CHAINS),
    "zeros300000": (lambda: bytes(300000), (262144, 1 << 20), (65535, 3)),
    "period1000": (lambda: (rnd(1000, 90) * 200)[:200000], (262144, 1 << 20), (65535, 3)),
}


def check_recorded(compressor, name, bs):
    make, block_sizes, chains = RECORDED[name]
    assert bs in block_sizes
    data = make()
    with open(os.path.join(ROOT, "tests", "golden", "emit_records.json")) as f:
        cases = [c for c in json.load(f)["cases"] if c["name"] == name and c["block_size"] == bs]
    assert sorted(c["max_chain"] for c in cases) == sorted(chains)
    for c in cases:
        assert hashlib.sha256(data).hexdigest() == c["input_sha256"]
        want = bytes.fromhex(c["frame_hex"])
        assert pyoracle.oz_unlz4(want) == data  # the recorded frame is a frame of this input
        got = compressor.compress_blocks(data, bs, c["max_chain"])
        assert got == want, (name, bs, c["max_chain"], len(got), len(want))


# ---- sub-segment edges: a walk sub-segment holds 4096 positions --------------------------------------------------
@pytest.mark.parametrize("n", [4095, 4096, 4097, 8191, 8192, 8193, 12289, 65535, 65536])
def test_sub_segment_edges(compressor, n):
    check(compressor, synth.enwik8_like(n, seed=1000 + n % 997), 65536)


def test_seventeen_sub_segments(compressor):
    """65537 bytes in one block: 17 sub-segments, the last of one position (the smallest slot capacity)."""
    check(compressor, synth.enwik8_like(65537, seed=1717), 262144)


# ---- a speculative walk that starts inside a match ---------------------------------------------------------------
def test_speculative_entry_inside_a_match(compressor):
    """One match from position ~57 to the block's end covers the first positions of sub-segments 1 .. 3: their
    speculative walks record matches the true path never takes, and the repair has to drop them all."""
    n = 3 * 4096 + 100
    unit = rnd(7, 21)
    data = rnd(50, 20) + (unit * (n // 7 + 1))[:n - 50]
    assert len(data) == n
    check(compressor, data, 65536)


# ---- long runs: one match spans whole sub-segments ----------------------------------------------------------------
@pytest.mark.parametrize("name", ["zeros20000", "zeros70000", "runs"])
def test_long_runs(compressor, name):
    if name in RECORDED:
        check_recorded(compressor, name, 65536)
    else:
        check(compressor, bytes(20000) if name == "zeros20000" else synth.runs(60000, seed=4, max_run=5000), 65536)


# ---- many tokens per sub-segment ---------------------------------------------------------------------------------
def test_many_tokens_per_sub_segment(compressor):
    """8 000 draws from 256 random 4-byte words, one random byte after each: a minimal match every five bytes,
    about 800 records per sub-segment (several 64-record batches, and repairs that move hundreds of entries)."""
    rng = np.random.default_rng(31)
    words = rng.integers(0, 256, (256, 4), dtype=np.uint8)
    draws = words[rng.integers(0, 256, 8000)]
    data = np.concatenate([draws, rng.integers(0, 256, (8000, 1), dtype=np.uint8)], axis=1).tobytes()
    assert len(data) == 40000
    check(compressor, data, 65536)


# ---- literal and match length codes -------------------------------------------------------------------------------
def test_literal_run_length_codes(compressor):
    """Literal runs of 14, 15, 16 (the token's escape), 64, 65 (kOwnLits: the wave-wide copy starts above 64),
    269, 270, 271 (the second extra byte) and 600 between matches of a 32-byte motif."""
    motif = rnd(32, 40)
    data = motif
    for i, L in enumerate((14, 15, 16, 64, 65, 269, 270, 271, 600)):
        data += rnd(L, 41 + i) + motif
    data += rnd(16, 60)
    check(compressor, data, 65536)


@pytest.mark.parametrize("k", [18, 19, 20, 273, 274, 275])
def test_match_length_codes(compressor, k):
    """A block that repeats its first k bytes: one match of k (codes 14, 15, 16 and the second extra byte)."""
    head = rnd(k, 70 + k)
    check(compressor, head + head + rnd(16, 71 + k), 65536)


# ---- stored and compressed blocks in one call ---------------------------------------------------------------------
def test_stored_and_compressed_blocks(compressor):
    data = rnd(65536, 80) + synth.enwik8_like(65536, seed=81) + rnd(100, 82)
    check(compressor, data, 65536, CHAINS + (0,))


# ---- wide fields: positions and lengths far above 16 bits ---------------------------------------------------------
@pytest.mark.parametrize("bs", [262144, 1 << 20])
@pytest.mark.parametrize("name", ["zeros300000", "period1000"])
def test_wide_fields(compressor, name, bs):
    """300 000 zero bytes (one match of nearly 2^18) and 200 000 bytes of period 1000, chains 65535 and 3.
    The period-1000 cases take 12.8 s each on an MI355X, all of it in the greedy level's match search at chain 3
    (chain 65535: 0.02 s), before the emit chain and the same with the commit before these tests."""
    check_recorded(compressor, name, bs)


# ---- the stream API goes through the same emit chain --------------------------------------------------------------
def test_stream_api_frames(compressor):
    data = synth.enwik8_like(10000, seed=95)
    dictionary = synth.enwik8_like(5000, seed=96)
    for chain in CHAINS:
        assert compressor.lz4(data, chain, b"", True) == pyoracle.oz_lz4(data, chain, b"", True), ("legacy", chain)
        assert compressor.lz4(data, chain, dictionary) == pyoracle.oz_lz4(data, chain, dictionary), ("dictionary", chain)
