"""The constructed parse cases (tests/golden/parsecases.py) on the CPU: what the case set lands on, and that
the oracle's stage-2 array is the thing the frame is made from.  No GPU here; tests/test_parse_choices.py
compares the device's per-position arrays with the same oracle arrays."""
import hashlib
import json
import os

import numpy as np
import pytest

import parse_oracle as po
import parsecases as pc
from oracle import pyoracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "parse_cases.json")

# the reference's search and parse are quadratic in a same-letter run wherever every position is searched: at
# levels 7 and up, and in stage 0 at any level (about 8 s per `same_letter` oracle call; the 600 000-byte block
# takes about 2.5 s).  Their tests are marked slow, and their census is taken at one level of each kind
HEAVY = ("same_letter", "many_segments")
CENSUS_LEVELS_HEAVY = (65535, 4, 1)
LIGHT = [c for c in po.base_cases() if c.family not in HEAVY]
HEAVY_CASES = [c for c in po.base_cases() if c.family in HEAVY]

# What the case set must keep landing on.  Written out, so that an edit of the builder cannot lose one
# silently.  Names are those of parsecases.census.
REQUIRED = {
    # a longest match (stage 0) of each length around the length-code extension points, the fast-batch
    # limit and kRmqLen
    "longest_18", "longest_19", "longest_64", "longest_65", "longest_273", "longest_274", "longest_528",
    "longest_529", "longest_783", "longest_784",
    # a chosen match on the emitted path of each length
    "path_match_4", "path_match_18", "path_match_19", "path_match_64", "path_match_65", "path_match_273",
    "path_match_274", "path_match_528", "path_match_529",
    # a literal run on the path of each length
    "path_lits_0", "path_lits_14", "path_lits_15", "path_lits_16", "path_lits_269", "path_lits_270", "path_lits_271",
    # a chosen length shorter than the longest: on the path and off it, the same with chosen >= 274, and > 64
    "short_on_path", "short_off_path", "short_rmq_on_path", "short_rmq_off_path", "short_above_64",
    # a parse segment without any match as top, middle and bottom segment
    "nomatch_segment_top", "nomatch_segment_middle", "nomatch_segment_bottom",
    # a chosen match across a parse-segment boundary, across a walk sub-segment boundary, over a whole segment
    "chosen_crosses_parse_boundary", "chosen_crosses_walk_boundary", "chosen_jumps_parse_segment",
    # a 64-position chunk whose lengths are all <= 64 next to one that holds a length > 64
    "chunk_le64_next_to_chunk_above_64",
    # a literal-length bump (15, 270) in the first and in the last 4-position batch of a chunk
    "bump_15_first_batch", "bump_15_last_batch", "bump_270_first_batch", "bump_270_last_batch",
    # a carried chain of at least 64 positions with full lengths, and a shortened one
    "chain_full_lengths", "chain_shortened",
    # same-letter matches around MaxSameLetter
    "same_letter_at_least_max", "same_letter_equal_max", "same_letter_max_minus_1", "same_letter_shortcut_interval",
    # a block of more than 64 parse segments with the rmq flag condition true (parallel repair), and its
    # partner of 64 segments (serial repair)
    "more_than_64_segments", "rmq_flag", "rmq_parallel_repair", "rmq_serial_repair",
    # the three-way edge of the stored/compressed decision
    "stored_enc_n", "stored_enc_n_plus_1", "compressed_enc_n_minus_1",
    # lazy levels: the skip bookkeeping cleared something; greedy levels: the lazy-evaluation position searched
    "lazy_stage1_differs", "greedy_lazy_eval_searched",
}
# wanted, not required (the census reports it): an optimum strictly inside a length piece k >= 1
WANTED = {"short_strictly_inside_piece"}
# the part of REQUIRED only the heavy families provide
HEAVY_ONLY = {"same_letter_at_least_max", "same_letter_equal_max", "same_letter_max_minus_1",
              "same_letter_shortcut_interval", "more_than_64_segments", "rmq_parallel_repair",
              "chosen_jumps_parse_segment"}


def census_of(case, chain):
    # at levels above the lazy ones nothing is skipped: stage 1 is stage 0
    l1, _ = po.stage(case, chain, 1)
    l0 = l1 if chain > pc.LAZY_MAX else po.stage(case, chain, 0)[0]
    l2, d = po.stage(case, chain, 2)
    return pc.census(case.data, l0, l1, l2, d, chain)


def test_case_set_shape():
    cases = po.base_cases()
    assert len({c.name for c in cases}) == len(cases)
    assert {c.family for c in cases} == {"edges", "junction", "periodic", "nomatch", "overlap_text", "same_letter",
                                         "many_segments", "stored_edge"}
    for c in cases:
        assert 65535 in c.levels
        if c.family in ("edges", "junction", "periodic", "nomatch", "overlap_text"):
            assert 12 * 1024 <= len(c.data) <= 24 * 1024, c
            assert 3 <= len(pc.dp_segments(len(c.data))) <= 6
        if c.family == "same_letter":
            assert len(c.data) == 128 * 1024
            assert set(c.levels) == {65535, 5} | set(pc.GREEDY) | set(pc.LAZY)   # 16, 8, 7: parsecases.base_cases
        else:
            assert set(c.levels) == set(pc.ALL_LEVELS)
        v = pc.variants(c)
        assert len(v) == (78 if c.family in pc.SWEPT else 0)
    assert len(pc.dp_segments(600000)) > 64 >= len(pc.dp_segments(64 * 8192))
    # deterministic
    again = pc.base_cases()
    assert [c.data for c in again] == [c.data for c in cases]


def test_census_light_cases_cover_their_share():
    """Everything but the heavy families' share of REQUIRED, from the 12-24 KiB cases and stored_edge."""
    seen = {}
    for c in LIGHT:
        for chain in c.levels:
            for name in census_of(c, chain):
                seen.setdefault(name, f"{c.name}@{chain}")
    missing = (REQUIRED - HEAVY_ONLY) - set(seen)
    assert not missing, sorted(missing)
    print("wanted:", {w: seen.get(w) for w in WANTED})


def test_junction_inside_has_optima_strictly_inside_a_length_piece():
    """The construction of junction_inside works: chosen lengths >= 274, shorter than the longest and not at
    the upper end of their 255-wide piece -- at the junctions themselves (on the path) and along the copies."""
    (c,) = [c for c in LIGHT if c.name == "junction_inside"]
    l1, l2 = po.stage(c, 65535, 1)[0], po.stage(c, 65535, 2)[0]
    assert "short_strictly_inside_piece" in census_of(c, 65535)
    assert pc.strictly_inside(l1, l2, len(c.data)) >= 1000
    on_path = [at for at, L in pc.path_of(l2, len(c.data)) if 274 <= L < l1[at] and (L - 18) % 255]
    assert len(on_path) >= 10, on_path


@pytest.mark.slow
def test_census_heavy_cases_cover_the_rest():
    jobs = [(c, chain) for c in HEAVY_CASES for chain in CENSUS_LEVELS_HEAVY]
    po.warm(jobs, stages=(0, 1, 2), blocks=False)
    seen = set()
    for c, chain in jobs:
        seen |= census_of(c, chain)
    assert not HEAVY_ONLY - seen, sorted(HEAVY_ONLY - seen)
    by = {c.name: census_of(c, 65535) for c in HEAVY_CASES}
    assert "rmq_parallel_repair" in by["many_segments_74"] and "rmq_serial_repair" in by["many_segments_64"]
    # the runs bracket MaxSameLetter: a run of r bytes gives its first searched position length r - 1
    assert "same_letter_max_minus_1" in by["same_letter_65299"] and "same_letter_at_least_max" not in by["same_letter_65299"]
    assert "same_letter_equal_max" in by["same_letter_65300"] and "same_letter_shortcut_interval" not in by["same_letter_65300"]
    assert "same_letter_shortcut_interval" in by["same_letter_65301"]
    assert not {n for n in by["same_letter_65298"] if n.startswith("same_letter")}


@pytest.mark.parametrize("case", [c for c in LIGHT if c.family in pc.SWEPT], ids=lambda c: c.name)
def test_census_sweeps_keep_the_content_and_move_the_boundaries(case):
    """Every variant keeps the base case's content features (the longest and chosen lengths; a trimmed block
    may lose what lay in its last 63 bytes, which is random filler), and over the trims every bump lands in
    the first and in the last batch of a chunk."""
    base = census_of(case, 65535)
    keep = {n for n in base if n.startswith(("longest_", "short_", "chain_"))}
    union = set()
    vs = pc.variants(case)
    po.warm([(v, 65535) for v in vs], stages=(1, 2), blocks=False)
    for v in vs:
        f = census_of(v, 65535)
        assert keep <= f, (v.name, sorted(keep - f))
        union |= f
    assert {"bump_15_first_batch", "bump_15_last_batch", "chosen_crosses_parse_boundary",
            "chosen_crosses_walk_boundary"} <= union


def check_choices_encode(case, chain):
    l2, d = po.stage(case, chain, 2)
    n = len(case.data)
    if chain > pc.GREEDY_MAX:
        assert int(l2[:max(n - pc.TAIL_LITS, 0)].min()) >= 1   # every parsed position holds a choice
    enc = pc.encode_choices(case.data, l2, d)
    blk = po.block(case, chain)
    word = int.from_bytes(blk[:4], "little")
    if word >> 31:
        assert len(enc) >= n and blk[4:] == case.data and word & 0x7FFFFFFF == n
    else:
        assert len(enc) < n and blk[4:] == enc and word == len(enc)


@pytest.mark.parametrize("case", LIGHT, ids=lambda c: c.name)
def test_stage2_choices_encode_to_the_payload(case):
    """Walking the stage-2 choices from position 0 and encoding them reproduces oz_block's payload."""
    for chain in case.levels:
        check_choices_encode(case, chain)


@pytest.mark.slow
def test_stage2_choices_encode_to_the_payload_heavy():
    po.warm([(c, chain) for c in HEAVY_CASES for chain in c.levels])
    for c in HEAVY_CASES:
        for chain in c.levels:
            check_choices_encode(c, chain)


def test_stored_edge_scripts_hit_their_deltas():
    """The fixed scripts give encLen = n - 1, n and n + 1 at level 65535, at every size; only n - 1 compresses."""
    for c in po.by_family("stored_edge"):
        want = pc.STORED_DELTA[c.name.rsplit("_", 1)[1]]
        l2, d = po.stage(c, 65535, 2)
        n = len(c.data)
        assert len(pc.encode_choices(c.data, l2, d)) - n == want, c.name
        assert po.block(c, 65535)[3] >> 7 == (0 if want < 0 else 1), c.name
        assert n in (300, 4000, 70000)
    assert len(po.by_family("stored_edge")) == 9


def stored_edge_search(n, seeds, copies):
    """(seed, copies) of the first script per delta in {-1, 0, 1}: how parsecases.STORED_EDGE was found."""
    found = {}
    for seed in seeds:
        for k in copies:
            data = pc.stored_edge_data(n, seed, k)
            l2, d = pyoracle.oz_block_matches(data, 65535, 2)
            delta = len(pc.encode_choices(data, l2, d)) - n
            if delta in (-1, 0, 1) and delta not in found:
                found[delta] = (n, seed, k)
        if len(found) == 3:
            break
    return found


def test_stored_edge_search_finds_the_fixed_scripts():
    for n in (300, 4000):   # (70 000 needs 94..103 copies: seeds 1..3, copies 90..110, two seconds)
        found = stored_edge_search(n, range(1, 40), range(0, 17))
        names = {-1: "m1", 0: "0", 1: "p1"}
        assert {names[k]: v for k, v in found.items()} == \
               {name.rsplit("_", 1)[1]: v for name, v in pc.STORED_EDGE.items() if v[0] == n}


def sha(b):
    return hashlib.sha256(b).hexdigest()


def fixture():
    with open(FIXTURE) as f:
        return {c["name"]: c for c in json.load(f)["cases"]}


def check_fixture(cases):
    fx = fixture()
    for c in cases:
        e = fx[c.name]
        assert e["input_len"] == len(c.data) and e["input_sha256"] == sha(c.data), c.name
        assert set(e["levels"]) == {str(x) for x in c.levels}
        for chain in c.levels:
            fr = po.frame(c, chain)
            assert (len(fr), sha(fr)) == (e["levels"][str(chain)]["frame_len"], e["levels"][str(chain)]["frame_sha256"]), \
                (c.name, chain)


def test_oracle_matches_the_reference_fixture():
    assert set(fixture()) == {c.name for c in po.base_cases()}
    assert os.path.getsize(FIXTURE) < 256 * 1024
    check_fixture(LIGHT)


@pytest.mark.slow
def test_oracle_matches_the_reference_fixture_heavy():
    po.warm([(c, chain) for c in HEAVY_CASES for chain in c.levels], stages=())
    check_fixture(HEAVY_CASES)


@pytest.mark.skipif(not pyoracle.ref_available(), reason="reference not compiled")
def test_light_cases_equal_the_live_reference():
    for c in LIGHT:
        for chain in c.levels:
            assert pyoracle.ref_lz4(c.data, chain) == po.frame(c, chain), (c.name, chain)


@pytest.mark.slow
@pytest.mark.skipif(not pyoracle.ref_available(), reason="reference not compiled")
def test_heavy_cases_equal_the_live_reference():
    from concurrent.futures import ThreadPoolExecutor
    jobs = [(c, chain) for c in HEAVY_CASES for chain in c.levels]
    po.warm(jobs, stages=())
    with ThreadPoolExecutor(max_workers=8) as ex:
        frames = list(ex.map(lambda j: pyoracle.ref_lz4(j[0].data, j[1]), jobs))
    for (c, chain), fr in zip(jobs, frames):
        assert fr == po.frame(c, chain), (c.name, chain)
