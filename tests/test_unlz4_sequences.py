"""The device decoder on blocks built from explicit sequence lists (tests/golden/lz4seq.py): field values
placed on the kernels' own boundaries -- overlap periods, length-extension edges, sequence counts, the
literal register window, the ring and its drains, matches below the block start, split mode's sub-segment
edges -- plus 40 seeded random frames and a few malformed ones.  Every comparison is byte for byte against
lz4seq.expand(), which tests/test_lz4seq_model.py pins to the oracle's decoder and to the reference's own.
Each well-formed case goes through every route that applies: the host API, a split-mode context, the batch
decoder (every block an item of its own, decoded from an all-zero history), device pointers at every frame
alignment, and the chunked stream decoder.  Run with -m gpu on an MI355X."""
import os
import struct

import pytest

import lz4seq
from smallz4_amd._native import NativeError

pytestmark = pytest.mark.gpu
FAMILIES = ["overlap", "lengths", "counts", "windows", "ring", "below", "split", "random"]
SENTINEL = 0xA5
PAD = 64


@pytest.fixture(scope="module")
def split(compressor):
    """A context whose decoder runs every frame in split mode (SZ4_UNLZ4_SPLIT=1)."""
    import smallz4_amd
    os.environ["SZ4_UNLZ4_SPLIT"] = "1"
    try:
        c = smallz4_amd.Compressor(device=0)
    finally:
        del os.environ["SZ4_UNLZ4_SPLIT"]
    yield c
    c.close()


@pytest.fixture(scope="module")
def expected():
    """expand() of every well-formed case, computed once."""
    return {repr(c): c.expected() for c in lz4seq.well_formed()}


def same(family, case, route, got, want):
    if got != want:
        n = min(len(got), len(want))
        at = next((i for i in range(n) if got[i] != want[i]), n)
        pytest.fail(f"{family}: {case} via {route}: {len(got)} bytes for {len(want)}, first difference at output "
                    f"offset {at}: {got[at:at + 8].hex()} for {want[at:at + 8].hex()}")


@pytest.mark.parametrize("family", FAMILIES)
def test_sequences_host_api(compressor, expected, family):
    """Compressor.unlz4: whole-block kernels (split mode only where a payload reaches kUnSplitMin)."""
    for case in lz4seq.well_formed(family):
        same(family, case, "unlz4", compressor.unlz4(case.frame(), case.dictionary), expected[repr(case)])


@pytest.mark.parametrize("family", FAMILIES)
def test_sequences_split_mode(split, expected, family):
    for case in lz4seq.well_formed(family):
        same(family, case, "split mode", split.unlz4(case.frame(), case.dictionary), expected[repr(case)])


@pytest.mark.parametrize("family", FAMILIES)
def test_sequences_batch(compressor, family):
    """unlz4_batch: every block an item of its own, decoded from an all-zero history -- a match below the
    block start reads zeros, never a neighbour item's output.  One call per family."""
    cases = [c for c in lz4seq.well_formed(family) if not c.dictionary]
    assert cases
    items, owners = [], []
    for case in cases:
        for k, (word, payload) in enumerate(case.items()):
            items.append(struct.pack("<I", word) + payload)
            owners.append((case, k))
    if family == "split":
        assert max(len(i) for i in items) - 4 >= 256 << 10  # one item of at least 256 KiB of payload
    got = compressor.unlz4_batch(items)
    assert len(got) == len(items)
    for (case, k), g in zip(owners, got):
        same(family, case, f"unlz4_batch item {k}", g, lz4seq.expand([case.blocks[k]], independent=True))


@pytest.mark.parametrize("family", FAMILIES)
def test_sequences_device_pointers(compressor, expected, family):
    """unlz4_device on slices of larger device tensors: every frame pointer alignment 0-7, an odd output
    pointer, sentinel bytes around the output left alone, and out_cap one byte short raising."""
    import torch
    cases = [c for c in lz4seq.well_formed(family) if c.device]
    assert cases
    for case in cases:
        frame, want = case.frame(), expected[repr(case)]
        fbuf = torch.zeros(len(frame) + 16, dtype=torch.uint8, device="cuda")
        obuf = torch.empty(len(want) + 2 * PAD + 16, dtype=torch.uint8, device="cuda")
        dbuf = torch.zeros(len(case.dictionary) + 16, dtype=torch.uint8, device="cuda")
        assert fbuf.data_ptr() % 8 == 0 and obuf.data_ptr() % 8 == 0 and dbuf.data_ptr() % 8 == 0
        ft = torch.frombuffer(bytearray(frame), dtype=torch.uint8).cuda()
        if case.dictionary:
            dbuf[3:3 + len(case.dictionary)] = torch.frombuffer(bytearray(case.dictionary), dtype=torch.uint8).cuda()
        d_dict = dbuf.data_ptr() + 3 if case.dictionary else 0
        for a in range(8):
            fbuf[a:a + len(frame)] = ft
            o = PAD + 1 + 2 * (a % 3)  # odd
            obuf.fill_(SENTINEL)
            n = compressor.unlz4_device(fbuf.data_ptr() + a, len(frame), obuf.data_ptr() + o, len(want), d_dict,
                                        len(case.dictionary))
            host = obuf.cpu().numpy().tobytes()
            assert n == len(want), (family, case, a)
            same(family, case, f"unlz4_device, frame pointer + {a}", host[o:o + n], want)
            assert host[:o] == bytes([SENTINEL]) * o, (family, case, a, "bytes before the output were written")
            assert host[o + n:] == bytes([SENTINEL]) * (len(host) - o - n), (family, case, a, "bytes after the output were written")
        with pytest.raises(NativeError):
            compressor.unlz4_device(fbuf.data_ptr() + 7, len(frame), obuf.data_ptr() + PAD + 1, len(want) - 1, d_dict,
                                    len(case.dictionary))


@pytest.mark.parametrize("family", FAMILIES)
def test_sequences_stream(compressor, expected, family):
    """unlz4_stream, the chunked decoder over callbacks, for the frames below 64 KiB (its read callback is
    per byte)."""
    for case in lz4seq.well_formed(family):
        frame = case.frame()
        if len(frame) >= 65536:
            continue
        it = iter(frame)
        out = []
        compressor.unlz4_stream(lambda: next(it, 0), out.append, case.dictionary)
        same(family, case, "unlz4_stream", b"".join(out), expected[repr(case)])


def test_sequences_malformed(compressor, split):
    """Every route reports the malformed cases (each rejected by the oracle, tests/test_lz4seq_model.py)."""
    import torch
    for case in lz4seq.malformed():
        frame = case.frame()
        with pytest.raises(NativeError):
            compressor.unlz4(frame)
        with pytest.raises(NativeError):
            split.unlz4(frame)
        with pytest.raises(NativeError):
            compressor.unlz4_batch([struct.pack("<I", word) + payload for word, payload in case.items()])
        f = torch.frombuffer(bytearray(frame), dtype=torch.uint8).cuda()
        out = torch.empty(1 << 20, dtype=torch.uint8, device="cuda")
        with pytest.raises(NativeError):
            compressor.unlz4_device(f.data_ptr(), len(frame), out.data_ptr(), out.numel())
        it = iter(frame)
        with pytest.raises(NativeError):
            compressor.unlz4_stream(lambda: next(it, 0), lambda b: None)
