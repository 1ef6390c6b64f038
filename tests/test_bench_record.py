"""CPU checks of the bench line's provenance: the roofline's `traffic` and issue rates come from the
newest committed PMC summary of the same workload (profiles/<tag>_pmc.json), tags ordered by round, then
r02a..r02z, r02aa..r02az, ... (a plain string sort would put r02o after r02bd, a length sort r03a before
r02bd)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (no GPU work at import)

DEFAULT_CFG = {"workload": "enwik8", "bytes_per_gpu": 100_000_000, "block_size": 65536, "level": 9}


def _tag_key(tag):
    return bench.pmc_tag_key(tag)


def test_tag_order():
    tags = ["r02o", "r02bd", "r03a", "r02av", "r03ab", "r03z", "r01h"]
    assert sorted(tags, key=_tag_key) == ["r01h", "r02o", "r02av", "r02bd", "r03a", "r03z", "r03ab"]


def test_pmc_traffic_takes_newest_tag_of_the_workload():
    got = bench.pmc_traffic(DEFAULT_CFG)
    assert got is not None
    path, rec = got
    tags = []
    for name in os.listdir(os.path.join(ROOT, "profiles")):
        if not name.endswith("_pmc.json"):
            continue
        with open(os.path.join(ROOT, "profiles", name)) as f:
            if json.load(f).get("config") == DEFAULT_CFG:
                tags.append(name[: -len("_pmc.json")])
    assert tags
    newest = max(tags, key=_tag_key)
    assert os.path.basename(path) == f"{newest}_pmc.json"
    # the record carries everything the roofline needs
    for k in ("avg_duration_us", "fetch_bytes_corrected", "write_bytes", "hbm_bytes_per_launch",
              "valu_per_simd_cycle", "salu_per_cu_cycle"):
        assert rec.get(k) is not None, k
    assert rec["hbm_bytes_per_launch"] == rec["fetch_bytes_corrected"] + rec["write_bytes"]


def test_plain_run_is_the_default_and_full_is_an_option():
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full


def test_dump_outputs_files(tmp_path):
    """--dump-outputs: float .npy files, the same from run to run, a sample above DUMP_SAMPLE bytes and
    chunk sums that show a change the sample does not hold."""
    import numpy as np
    n = bench.DUMP_SAMPLE + 100_001
    frame = np.random.default_rng(5).integers(0, 256, n, dtype=np.uint8)
    bench.dump_outputs(str(tmp_path / "a"), frame, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), frame, 0, 1)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["frame_chunk_sums.npy", "frame_sample.npy", "frame_size.npy"]
    a = {k: np.load(tmp_path / "a" / k) for k in names}
    for k in names:
        assert a[k].dtype in (np.float32, np.float64)
        assert np.array_equal(a[k], np.load(tmp_path / "b" / k))
    assert a["frame_size.npy"][0] == n and a["frame_sample.npy"].size == bench.DUMP_SAMPLE
    assert a["frame_chunk_sums.npy"][:, 0].sum() == int(frame.sum(dtype=np.uint64))
    # one byte changed at a position outside the sample
    held = np.zeros(n, dtype=bool)
    held[np.random.default_rng(bench.DUMP_SEED).integers(0, n, bench.DUMP_SAMPLE)] = True
    pos = int(np.flatnonzero(~held)[0])
    other = frame.copy()
    other[pos] ^= 1
    bench.dump_outputs(str(tmp_path / "c"), other, 0, 1)
    assert np.array_equal(a["frame_sample.npy"], np.load(tmp_path / "c" / "frame_sample.npy"))
    assert not np.array_equal(a["frame_chunk_sums.npy"], np.load(tmp_path / "c" / "frame_chunk_sums.npy"))
    # a small frame is written whole; ranks of a sharded run write their own files
    bench.dump_outputs(str(tmp_path / "d"), frame[:1000], 1, 2)
    assert np.array_equal(np.load(tmp_path / "d" / "frame_sample_rank1.npy"), frame[:1000].astype(np.float32))


def test_pmc_traffic_none_for_unprofiled_workload():
    assert bench.pmc_traffic(dict(DEFAULT_CFG, level=3)) is None
