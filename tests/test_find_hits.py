"""The -9 finder's hit path (k_find_sorted): constructed key groups whose layout over the sorted slots is
checked on the CPU with a model of the sort -- slots ascend by (16-bit multiplicative hash of the four
key bytes, position), chunks are 64 fixed slots -- before the GPU's per-position matches are compared with
the oracle's exhaustive search and the frame with the oracle's.

The model leaves out the block's last three positions (their keys read past the block), so a true slot is
the model's plus 0..3: every layout property is asserted for each of these shifts."""
import functools

import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import synth

HDR = bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x70, 0xDF])
N = 60000 + 37           # the last chunk holds fewer than 64 slots
KA = bytes([0x81, 0x92, 0xA3, 0xB4])   # keys of bytes >= 0x80 never occur in the text
KB = bytes([0xC5, 0xD6, 0xE7, 0xF8])
SHIFTS = range(4)


def _hash16(keys):
    return ((keys.astype(np.uint64) * 2654435761) & 0xFFFFFFFF) >> 16


def _slots(block):
    """Model slot of every position but the last three."""
    b = np.frombuffer(block, dtype=np.uint8).astype(np.uint32)
    keys = b[:-3] | (b[1:-2] << 8) | (b[2:-1] << 16) | (b[3:] << 24)
    pos = np.arange(len(keys))
    order = np.lexsort((pos, _hash16(keys)))
    slot = np.empty(len(keys), dtype=np.int64)
    slot[order] = pos
    return slot


def _lcp(block, a, b, stop):
    k = 0
    while b + k < stop and block[a + k] == block[b + k]:
        k += 1
    return k


@functools.lru_cache(maxsize=None)
def _colliding_keys():
    """Two different 4-byte keys (bytes >= 0x80) with the same 16-bit hash, found by search."""
    rng = np.random.default_rng(5)
    raw = rng.integers(0x80, 0x100, size=(200000, 4), dtype=np.uint32)
    keys = raw[:, 0] | (raw[:, 1] << 8) | (raw[:, 2] << 16) | (raw[:, 3] << 24)
    h = _hash16(keys)
    seen = {}
    for k, hv in zip(keys.tolist(), h.tolist()):
        if hv in seen and seen[hv] != k:
            return seen[hv].to_bytes(4, "little"), k.to_bytes(4, "little")
        seen[hv] = k
    raise AssertionError("no colliding pair found")


def _put(buf, at, rec):
    buf[at:at + len(rec)] = rec


def _uniq(i):
    return bytes([0x30 + (i // 10) % 10, 0x30 + i % 10, 0x40 + (i * 7) % 26, 0x61 + (i * 11) % 26])


@functools.lru_cache(maxsize=None)
def _block(mirror):
    """Text with four planted key groups; returns (block, marks)."""
    buf = bytearray(synth.enwik8_like(N, seed=41))
    marks = {}
    # group A: 100 records of key KA, 500 bytes apart: more than one chunk.  The last one is the target;
    # record 97 (same chunk) and record 10 (a chunk below) share its first 10 bytes -- the mirror case
    # gives record 10 one byte more
    stem = KA + b"ABCDEF"
    for i in range(100):
        _put(buf, 100 + 500 * i, KA + bytes([0x35]) + _uniq(i) + b"....")
    tgt, c1, c2 = 100 + 500 * 99, 100 + 500 * 97, 100 + 500 * 10
    _put(buf, tgt, stem + b"xu--")
    _put(buf, c1, stem + b"yv--")
    _put(buf, c2, stem + (b"xw--" if mirror else b"zw--"))
    marks.update(tgt=tgt, c1=c1, c2=c2)
    # group B: 40 records of key KB with 16 more equal bytes, then a common continuation of varying length:
    # every in-chunk candidate is equal on 12 bytes and must be extended from the text
    body = b"0123456789abcdef"
    cont = b"ZYXWVUTSRQ"
    marks["b"] = []
    for j in range(40):
        at = 300 + 500 * j
        _put(buf, at, KB + body + cont[:(j * 3) % 10] + _uniq(j + 50) + b"!")
        marks["b"].append(at)
    # two keys of one hash group, interleaved by position; records of the same key share 7 bytes
    k3, k4 = _colliding_keys()
    marks["kk"] = []
    for j in range(24):
        at = 50000 + 150 * j
        _put(buf, at, (k3 if j % 2 == 0 else k4) + b"mno" + _uniq(j + 20))
        marks["kk"].append(at)
    # a target of group A whose limit is below 12: the last searched position of the block
    last = N - 12
    _put(buf, last, stem + b"xu"[:2])
    marks["last"] = last
    return bytes(buf), marks


def _check_layout(block, marks, mirror):
    slot = _slots(block)
    stop = len(block) - 5
    tgt, c1, c2 = marks["tgt"], marks["c1"], marks["c2"]
    akey = [p for p in range(len(block) - 3) if block[p:p + 4] == KA]
    for d in SHIFTS:
        # the target's chunk holds c1 and not c2
        assert (slot[tgt] + d) // 64 == (slot[c1] + d) // 64 > (slot[c2] + d) // 64
        # group A straddles a chunk boundary, members on both sides
        chunks = {(slot[p] + d) // 64 for p in akey}
        assert len(chunks) >= 2
        # more than 64 queue entries in one chunk of group B: m members give m (m - 1) / 2
        bs = np.array([(slot[p] + d) // 64 for p in marks["b"]])
        m = np.bincount(bs - bs.min()).max()
        assert m * (m - 1) // 2 > 64
    # in-chunk candidates of the target (between c2's chunk end and the target) and the ones below
    inch = [p for p in akey if p < tgt and slot[p] // 64 == slot[tgt] // 64]
    below = [p for p in akey if p < tgt and slot[p] // 64 < slot[tgt] // 64]
    li = max(_lcp(block, p, tgt, stop) for p in inch)
    lb = max(_lcp(block, p, tgt, stop) for p in below)
    assert _lcp(block, c1, tgt, stop) == li and _lcp(block, c2, tgt, stop) == lb
    assert lb == li + 1 if mirror else lb == li
    # the colliding keys: one hash, two keys, alternating
    k3, k4 = _colliding_keys()
    assert k3 != k4 and _hash16(np.array([int.from_bytes(k3, "little")]))[0] == \
        _hash16(np.array([int.from_bytes(k4, "little")]))[0]
    s = [slot[p] for p in marks["kk"]]
    assert s == sorted(s) and s[-1] - s[0] < len(s) + 4  # one hash group, ordered by position
    # the last chunk is partial; the last searched target has room for fewer than 12 bytes
    assert len(block) % 64 != 0
    assert stop - marks["last"] < 12 and block[marks["last"]:marks["last"] + 4] == KA


def _check(compressor, block, bs=65536):
    ol, od = pyoracle.oz_block_matches(block, 65535, 0)
    try:
        compressor.debug_stop_after(3)
        compressor.compress_blocks(block, bs, 65535)
        gl, gd = compressor.debug_matches(len(block))
    finally:
        compressor.debug_stop_after(0)
    n = len(block) - 11
    assert (gl[:n] == ol[:n]).all(), np.nonzero(gl[:n] != ol[:n])[0][:8]
    assert (gd[:n][ol[:n] > 0] == od[:n][ol[:n] > 0]).all()
    assert compressor.compress_blocks(block, bs, 65535) == HDR + pyoracle.oz_block(block, 65535) + b"\0\0\0\0"
    return ol, od


@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True], ids=["tie", "below_longer"])
def test_constructed_groups(compressor, mirror):
    block, marks = _block(mirror)
    _check_layout(block, marks, mirror)
    ol, od = _check(compressor, block)
    # the oracle agrees with the construction: the nearest of the longest wins
    tgt = marks["tgt"]
    assert ol[tgt] == (11 if mirror else 10)
    assert od[tgt] == tgt - (marks["c2"] if mirror else marks["c1"])
    assert ol[marks["last"]] == len(block) - 5 - marks["last"]


@pytest.mark.gpu
def test_groups_with_window_test_large_block(compressor):
    """The same groups twice in one 128 KiB block: the second segment's window is wider than 64 KiB, so
    the finder tests every candidate against the target's window."""
    a, _ = _block(False)
    b, _ = _block(True)
    block = a + synth.enwik8_like(65536 - len(a) + 11, seed=43) + b
    assert len(block) > 65536 + len(a)
    _check(compressor, block, 131072)


@pytest.mark.gpu
def test_groups_in_dependent_stream_block(compressor):
    """The groups at the end of a stream's first block and again in its second: the second block's
    candidates reach back into the first, and the lookback cut applies."""
    M = 4 << 20
    a, _ = _block(False)
    b, _ = _block(True)
    data = synth.enwik8_like(M - len(a), seed=42) + a + b[:40960]
    assert len(data) == M + 40960
    assert compressor.lz4(data, 65535) == pyoracle.oz_lz4(data, 65535)
