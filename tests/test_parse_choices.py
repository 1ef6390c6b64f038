"""Per-position parity of the parse with the oracle on the constructed cases of tests/golden/parsecases.py.

The frame shows the parse's choices only where the emitted path passes; `k_dp_spec_*` / `k_dp_fix<*>` compute a
choice for EVERY position.  Here the device's whole `sel` array (debug_stop_after(4) + debug_matches) is
compared with the oracle's stage 2, and at greedy/lazy levels the match arrays after the skip bookkeeping
with stage 1.  No position is masked and no class of positions is excluded: the comparison covers every
position below n - 5 of every case.  Run with -m gpu on an MI355X."""
import hashlib
import json
import os

import numpy as np
import pytest

import parse_oracle as po
import parsecases as pc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILIES = ["edges", "junction", "periodic", "nomatch", "overlap_text", "stored_edge", "same_letter", "many_segments"]
SWEPT_CASES = [c for c in po.base_cases() if c.family in pc.SWEPT]
PARSED = lambda c: [x for x in c.levels if x > pc.GREEDY_MAX]                      # noqa: E731
GREEDY_LAZY = lambda c: [x for x in c.levels if x <= pc.LAZY_MAX]                  # noqa: E731


def stopped_after_parse(compressor, data, chain, parse_input=False):
    """(len, dist) per position after the parse stage of one block holding all of `data`."""
    try:
        compressor.debug_stop_after(4)
        compressor.compress_blocks(data, len(data), chain)
        return compressor.debug_matches(len(data), parse_input=parse_input)
    finally:
        compressor.debug_stop_after(0)


def describe(name, chain, got, want, l1):
    bad = np.flatnonzero(got != want)
    on = np.zeros(len(want), dtype=bool)
    for at, _ in pc.path_of(want, len(want)):
        on[at] = True
    head = ", ".join(f"{p}: device {got[p]} oracle {want[p]} longest {l1[p]}{' (on path)' if on[p] else ''}" for p in bad[:8])
    return f"{name} at level {chain}: {len(bad)} positions differ ({int(on[bad].sum())} on the path): {head}"


def check_choices(compressor, case, chain):
    """sel equals oracle stage 2 at every position below n - 5, distances wherever a match was chosen."""
    n = len(case.data)
    ol, od = po.stage(case, chain, 2)
    gl, gd = stopped_after_parse(compressor, case.data, chain)
    top = n - pc.TAIL_LITS
    if not (gl[:top] == ol[:top]).all():
        pytest.fail(describe(case.name, chain, gl[:top], ol[:top], po.stage(case, chain, 1)[0]))
    m = ol[:top] > 1
    assert (gd[:top][m] == od[:top][m]).all(), (case.name, chain)


def check_stage1(compressor, case, chain):
    """The match arrays after the greedy/lazy skip bookkeeping equal oracle stage 1 at every position;
    distances wherever the reference searched and found a match."""
    ol, od = po.stage(case, chain, 1)
    gl, gd = stopped_after_parse(compressor, case.data, chain, parse_input=chain > pc.GREEDY_MAX)
    if not (gl == ol).all():
        pytest.fail(describe(case.name, chain, gl, ol, ol))
    m = ol > 1
    assert (gd[m] == od[m]).all(), (case.name, chain)


def check_frame(compressor, case, chain):
    want = po.frame(case, chain)
    got = compressor.compress_blocks(case.data, len(case.data), chain)
    assert got == want, (case.name, chain, len(got), len(want))
    assert compressor.unlz4(got) == case.data, (case.name, chain)


# ---- a. the parse's choices -------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_choices_base_cases(compressor, family):
    cases = po.by_family(family)
    po.warm([(c, chain) for c in cases for chain in PARSED(c)], stages=(2,), blocks=False)
    for c in cases:
        for chain in PARSED(c):
            check_choices(compressor, c, chain)


@pytest.mark.parametrize("case", SWEPT_CASES, ids=lambda c: c.name)
def test_choices_sweeps(compressor, case):
    """The 63 end-trimmed and 15 front-padded variants of a swept base case, at level 65535."""
    vs = pc.variants(case)
    po.warm([(v, 65535) for v in vs], stages=(2,), blocks=False)
    for v in vs:
        check_choices(compressor, v, 65535)


# ---- b. stage 1 at greedy and lazy levels -----------------------------------------------------------
@pytest.mark.parametrize("family", [f for f in FAMILIES if any(GREEDY_LAZY(c) for c in po.by_family(f))])
def test_stage1_greedy_lazy(compressor, family):
    cases = po.by_family(family)
    jobs = [(c, chain) for c in cases for chain in GREEDY_LAZY(c)]
    po.warm(jobs, stages=(1,), blocks=False)
    for c, chain in jobs:
        check_stage1(compressor, c, chain)


# ---- c. frames ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_frames_base_cases(compressor, family):
    cases = po.by_family(family)
    po.warm([(c, chain) for c in cases for chain in c.levels], stages=())
    for c in cases:
        for chain in c.levels:
            check_frame(compressor, c, chain)


@pytest.mark.parametrize("case", SWEPT_CASES, ids=lambda c: c.name)
def test_frames_sweeps(compressor, case):
    """The variants' frames at 65535, one lazy and one greedy level (parsecases.SWEEP_LEVELS)."""
    vs = pc.variants(case)
    po.warm([(v, chain) for v in vs for chain in v.levels], stages=())
    for v in vs:
        for chain in v.levels:
            check_frame(compressor, v, chain)


@pytest.mark.parametrize("chain", pc.ALL_LEVELS)
def test_frames_as_one_batch(compressor, chain):
    """Every base case meant for the level as an item of ONE compress_batch call: many different n at once."""
    cases = [c for c in po.base_cases() if chain in c.levels]
    po.warm([(c, chain) for c in cases], stages=())
    got = compressor.compress_batch([c.data for c in cases], chain)
    for c, blk in zip(cases, got):
        assert blk == po.block(c, chain), (c.name, chain)


def test_stored_edge_size_words(compressor):
    """encLen = n - 1 compresses; n and n + 1 are stored (the reference stores unless encLen < size)."""
    for c in po.by_family("stored_edge"):
        delta = pc.STORED_DELTA[c.name.rsplit("_", 1)[1]]
        n = len(c.data)
        frame = compressor.compress_blocks(c.data, n, 65535)
        word = int.from_bytes(frame[7:11], "little")
        if delta < 0:
            assert word >> 31 == 0 and word == n - 1 and len(frame) == 7 + 4 + n - 1 + 4, c.name
        else:
            assert word >> 31 == 1 and word & 0x7FFFFFFF == n and frame[11:11 + n] == c.data, c.name
        assert frame == po.frame(c, 65535), c.name


def test_base_cases_match_the_reference_fixture(compressor):
    """Level 65535 against the reference's own frames (tests/golden/parse_cases.json): length and SHA-256."""
    with open(os.path.join(ROOT, "tests", "golden", "parse_cases.json")) as f:
        fx = {c["name"]: c for c in json.load(f)["cases"]}
    for c in po.base_cases():
        e = fx[c.name]
        assert e["input_sha256"] == hashlib.sha256(c.data).hexdigest(), c.name
        frame = compressor.compress_blocks(c.data, len(c.data), 65535)
        want = e["levels"]["65535"]
        assert (len(frame), hashlib.sha256(frame).hexdigest()) == (want["frame_len"], want["frame_sha256"]), c.name
