"""The oracle's arrays and blocks of the constructed parse cases, computed once per test session.

tests/test_parse_model.py and tests/test_parse_choices.py share this cache, so no assertion recomputes an
oracle array.  `warm` fills it for a list of (case, level) on a thread pool (ctypes releases the GIL): the
reference's search and parse are quadratic in a same-letter run, and the four `same_letter` cases take
several seconds each on one core.
"""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import parsecases
from oracle import pyoracle

HDR = bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x70, 0xDF])
_cache: dict = {}
_base = None


def base_cases():
    global _base
    if _base is None:
        _base = parsecases.base_cases()
    return _base


def by_family(family: str):
    return [c for c in base_cases() if c.family == family]


def stage(case, chain: int, st: int):
    """(len, dist) of oz_block_matches(case.data, chain, st); read-only."""
    key = (case.name, chain, st)
    if key not in _cache:
        ln, ds = pyoracle.oz_block_matches(case.data, chain, st)
        ln.setflags(write=False)
        ds.setflags(write=False)
        _cache[key] = (ln, ds)
    return _cache[key]


def block(case, chain: int) -> bytes:
    """Size word + payload of the case compressed on its own."""
    key = (case.name, chain, "block")
    if key not in _cache:
        _cache[key] = pyoracle.oz_block(case.data, chain)
    return _cache[key]


def frame(case, chain: int) -> bytes:
    return HDR + block(case, chain) + b"\0\0\0\0"


def warm(jobs, stages=(2,), blocks=True, workers: int = 8):
    """Fill the cache for every (case, chain) of jobs."""
    todo = [(c, ch, st) for c, ch in jobs for st in stages if (c.name, ch, st) not in _cache]
    todo += [(c, ch, "block") for c, ch in jobs if blocks and (c.name, ch, "block") not in _cache]
    if not todo:
        return
    with ThreadPoolExecutor(max_workers=workers) as ex:
        list(ex.map(lambda t: block(t[0], t[1]) if t[2] == "block" else stage(*t), todo))
