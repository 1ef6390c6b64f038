"""The typed ragged batch API on the GPU: every item is split into its byte planes while it is staged and
merged again after the batch decoder.  Expected bytes come only from the oracle on the host model's split
(oz_block(planes.split(item, E))) and from the items themselves; every comparison is byte-for-byte.
Run with -m gpu on an MI355X."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import _native, planes, synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8)


def sizes_for(E):
    return [0, 1, E - 1, E, E + 1, 15, 16, 17, 16 * E - 1, 16 * E, 16 * E + 1, 255, 256, 257, 1000, 4095, 4096, 4097,
            65535, 65536, 65537, 70001, 200003]


def oracle_blocks(items, chain):
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda x: pyoracle.oz_block(x, chain), items))


def numeric_bytes(n, seed):
    """Typed-looking bytes: increasing int32 counters, then increasing int64 ones.  The steps are large enough
    that no byte plane is one long run (the oracle takes seconds per item on those), small enough that the upper
    planes repeat."""
    rng = np.random.default_rng(seed)
    a = (np.cumsum(rng.integers(0, 70000, n // 8 + 8)) & 0x7FFFFFFF).astype(np.int32).tobytes()
    b = np.cumsum(rng.integers(0, 2 ** 44, n // 16 + 8, dtype=np.int64)).astype(np.int64).tobytes()
    return (a + b)[:n]


@functools.lru_cache(maxsize=None)
def typed_case():
    """(buffer, ((offset, size, E), ...)): the items are slices of one buffer (text, then numeric data); the
    k-th non-empty item starts at source alignment k mod 16, so they cover every alignment several times.
    After the sizes of every width come a random item (stored) and an all-zero item."""
    spec = [(n, E) for E in WIDTHS for n in sizes_for(E)] + [(5000, 4), (5000, 2)]
    slices, at, k = [], 0, 0
    for n, E in spec:
        if n:
            at += (k - at) % 16
            k += 1
        slices.append((at, n, E))
        at += n
    half = at // 2
    buf = bytearray(synth.enwik8_like(half, seed=61) + numeric_bytes(at + 64 - half, seed=62))
    a, n, _ = slices[-2]
    buf[a:a + n] = synth.random_bytes(n, seed=63)
    a, n, _ = slices[-1]
    buf[a:a + n] = bytes(n)
    return bytes(buf), tuple(slices)


def case_items():
    buf, slices = typed_case()
    return [buf[a:a + n] for a, n, _ in slices]


@functools.lru_cache(maxsize=None)
def case_split():
    buf, slices = typed_case()
    return tuple(planes.split(buf[a:a + n], E) for a, n, E in slices)


@functools.lru_cache(maxsize=None)
def case_expected(chain):
    return tuple(oracle_blocks(list(case_split()), chain))


def device_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


_gpu_blocks = {}


def gpu_case(comp, chain):
    """The case compressed by the typed call: (raw bytes, offsets), once per chain."""
    if chain not in _gpu_blocks:
        import torch
        buf, slices = typed_case()
        base = device_bytes(buf)
        assert {(base.data_ptr() + a) % 16 for a, n, _ in slices if n} == set(range(16))
        sizes = [n for _, n, _ in slices]
        ptrs = [base.data_ptr() + a if n else 0 for a, n, _ in slices]
        elems = [E for _, _, E in slices]
        cap = comp.batch_bound(sizes)
        out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        off = comp.compress_batch_typed_device(ptrs, sizes, elems, out.data_ptr(), cap, chain)
        sizes_reported = comp.last_block_sizes(len(sizes))
        _gpu_blocks[chain] = (out[:off[-1]].cpu().numpy().tobytes(), off, sizes_reported)
    return _gpu_blocks[chain]


# ---- 1. parity -------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [0, 3, 7, 65535])
def test_typed_parity(compressor, chain):
    _, slices = typed_case()
    raw, off, reported = gpu_case(compressor, chain)
    want = case_expected(chain)
    assert len(off) == len(slices) + 1 and off[0] == 0
    for i, (a, n, E) in enumerate(slices):
        assert raw[off[i]:off[i + 1]] == want[i], f"item {i} ({n} bytes, width {E}) differs at chain {chain}"
    assert reported == [len(w) for w in want]
    if chain == 0:  # a stored block is the size word and the split bytes: the gather alone
        for i, s in enumerate(case_split()):
            assert raw[off[i]:off[i + 1]] == ((len(s) | 0x80000000).to_bytes(4, "little") + s if s else b"")


# ---- 2. identity at width 1 ------------------------------------------------------------------
def test_width_one_is_the_plain_call(compressor):
    import torch
    buf, slices = typed_case()
    base = device_bytes(buf)
    sizes = [n for _, n, _ in slices]
    ptrs = [base.data_ptr() + a if n else 0 for a, n, _ in slices]
    cap = compressor.batch_bound(sizes)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    off = compressor.compress_batch_device(ptrs, sizes, out.data_ptr(), cap, 7)
    plain = out[:off[-1]].cpu().numpy().tobytes()
    out.zero_()
    off1 = compressor.compress_batch_typed_device(ptrs, sizes, [1] * len(sizes), out.data_ptr(), cap, 7)
    assert off1 == off
    assert out[:off[-1]].cpu().numpy().tobytes() == plain


# ---- 3. typed blocks are ordinary blocks -----------------------------------------------------
def test_typed_blocks_decode_to_the_split(compressor):
    raw, off, _ = gpu_case(compressor, 3)
    blocks = [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    assert compressor.unlz4_batch(blocks) == list(case_split())


# ---- 4. round trip ---------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [33, 64])  # d_out at an odd address, and at an aligned one
def test_round_trip(compressor, lead):
    import torch
    items = case_items()
    elems = [E for _, _, E in typed_case()[1]]
    raw, off, _ = gpu_case(compressor, 7)
    d = device_bytes(raw)
    want_off = [0]
    for x in items:
        want_off.append(want_off[-1] + len(x))
    total = want_off[-1]
    assert compressor.unlz4_batch_typed_device(d.data_ptr(), off, elems, 0, 0) == want_off  # query mode
    buf = torch.full((lead + total + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_out = buf.data_ptr() + lead
    assert d_out % 2 == lead % 2
    # one byte short: SZ4_E_CAPACITY, the offsets filled in, nothing written
    o = (ctypes.c_uint64 * len(off))(*off)
    w = (ctypes.c_uint8 * len(elems))(*elems)
    res = (ctypes.c_uint64 * len(off))()
    rc = compressor._lib.sz4_unlz4_batch_typed_device(compressor._h, ctypes.c_void_p(d.data_ptr()), o, w, len(elems),
                                                      ctypes.c_void_p(d_out), total - 1, res, None)
    assert rc == _native.SZ4_E_CAPACITY
    assert list(res) == want_off
    assert bool((buf == 0xA5).all())
    got_off = compressor.unlz4_batch_typed_device(d.data_ptr(), off, elems, d_out, total)
    assert got_off == want_off
    host = buf.cpu().numpy().tobytes()
    assert host[:lead] == b"\xA5" * lead and host[lead + total:] == b"\xA5" * 64
    for i, x in enumerate(items):
        assert host[lead + want_off[i]:lead + want_off[i + 1]] == x, f"item {i} ({len(x)} bytes, width {elems[i]})"
    assert compressor.unlz4_batch_typed([raw[off[i]:off[i + 1]] for i in range(len(items))], elems) == items


# ---- 5. several pieces -----------------------------------------------------------------------
def test_pieces_give_the_same_bytes(compressor):
    import smallz4_amd
    data = synth.enwik8_like(1 << 20, seed=64) + numeric_bytes(2 << 20, seed=65)
    base = device_bytes(data)
    rng = np.random.default_rng(66)
    items, elems, at = [], [], 0
    while at < len(data):
        n = min(int(rng.integers(20_000, 150_000)), len(data) - at)
        items.append(base[at:at + n])
        elems.append(WIDTHS[len(items) % 4])
        at += n
    one = compressor.compress_batch_typed(items, elems, 7)
    comp = smallz4_amd.Compressor(device=0)
    try:
        comp.set_batch_chunk(1 << 20)
        assert comp.compress_batch_typed(items, elems, 7) == one
    finally:
        comp.close()
    k = len(items) // 2
    assert one[k] == pyoracle.oz_block(planes.split(items[k].cpu().numpy().tobytes(), elems[k]), 7)


# ---- 6. one large item -----------------------------------------------------------------------
def test_one_large_item(compressor):
    n = (4 << 20) - 3
    item = numeric_bytes(n + 3, seed=67)[3:]
    blocks = compressor.compress_batch_typed([item], [8], 3)
    assert blocks[0] == pyoracle.oz_block(planes.split(item, 8), 3)
    assert len(blocks[0]) < n  # not stored
    assert compressor.unlz4_batch_typed(blocks, [8]) == [item]


# ---- 7. errors -------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [3, 0])
def test_bad_width_is_refused(compressor, bad):
    import torch
    d = device_bytes(synth.enwik8_like(3000, seed=68))
    out = torch.full((4000,), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):  # SZ4_E_ARG
        compressor.compress_batch_typed_device([d.data_ptr(), d.data_ptr() + 1000], [1000, 2000], [4, bad], out.data_ptr(),
                                               4000, 7)
    assert bool((out == 0xA5).all())
    block = pyoracle.oz_block(planes.split(bytes(1000), 4), 7)
    b = device_bytes(block)
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):
        compressor.unlz4_batch_typed_device(b.data_ptr(), [0, len(block)], [bad], out.data_ptr(), 4000)
    assert bool((out == 0xA5).all())
    with pytest.raises(TypeError):
        compressor.compress_batch_typed([b"abcdef"], [bad])
    with pytest.raises(TypeError):
        compressor.compress_batch_typed([b"abcdef"])  # a bytes-like needs its width
    assert compressor.unlz4_batch_typed([block], [4]) == [bytes(1000)]


def test_corrupt_block_is_rejected_as_by_the_plain_decoder(compressor):
    text = synth.enwik8_like(5000, seed=69)
    a, b = pyoracle.oz_block(planes.split(text[:3000], 4), 65535), pyoracle.oz_block(planes.split(text[3000:], 2), 65535)
    d = device_bytes(a + b)
    bad_extent = [0, len(a) + 1, len(a) + len(b)]
    # and a malformed block of the decoder's conformance cases (tests/golden/lz4seq.py)
    import lz4seq
    word, payload = lz4seq.malformed()[0].items()[0]
    broken = word.to_bytes(4, "little") + payload
    m = device_bytes(broken)
    for offsets, ptr, elems in ((bad_extent, d.data_ptr(), [4, 2]), ([0, len(broken)], m.data_ptr(), [8])):
        codes = []
        for call in (lambda: compressor.unlz4_batch_device(ptr, offsets, 0, 0),
                     lambda: compressor.unlz4_batch_typed_device(ptr, offsets, elems, 0, 0)):
            with pytest.raises(_native.NativeError) as err:
                call()
            codes.append(str(err.value).split(")")[0].split("(")[-1])
        assert codes == ["-6", "-6"]  # SZ4_E_CORRUPT from both
    assert compressor.unlz4_batch_typed([a, b], [4, 2]) == [text[:3000], text[3000:]]


# ---- 8. tensors ------------------------------------------------------------------------------
def tensor_cases():
    import torch
    rng = np.random.default_rng(70)
    ids = np.sort(rng.integers(0, 5_000_000, 40_000)).astype(np.int32)
    stamps = (1_700_000_000_000 + np.cumsum(rng.integers(1, 1000, 20_000))).astype(np.int64)
    return {
        "bf16": torch.from_numpy(rng.normal(0, 0.02, 100_003).astype(np.float32)).to(torch.bfloat16),
        "fp32": torch.from_numpy(rng.normal(0, 0.02, (257, 129)).astype(np.float32)),
        "ids": torch.from_numpy(ids),
        "stamps": torch.from_numpy(stamps),
        "view": torch.from_numpy(rng.normal(0, 1, (96, 80)).astype(np.float32)).t()[:, ::2],
        "empty": torch.empty((0, 3), dtype=torch.float16),
        "uint8": torch.from_numpy(rng.integers(0, 7, 100_001, dtype=np.uint8)),
    }


@pytest.mark.parametrize("name", ["bf16", "fp32", "ids", "stamps", "view", "empty", "uint8"])
def test_tensor_round_trip(compressor, name):
    import torch
    t = tensor_cases()[name].cuda(0)
    if name == "view":
        assert not t.is_contiguous()
    ct = compressor.compress_tensor(t)
    assert ct.blocks.is_cuda and ct.blocks.dtype == torch.uint8 and ct.blocks.numel() == ct.offsets[-1]
    assert ct.dtype == t.dtype and ct.shape == tuple(t.shape) and ct.chunk_bytes == 65536
    back = compressor.decompress_tensor(ct)
    assert back.is_cuda and back.dtype == t.dtype and back.shape == t.shape
    same = back.contiguous().reshape(-1).view(torch.uint8) == t.contiguous().reshape(-1).view(torch.uint8)
    assert bool(same.all())


def test_sorted_ids_tensor_against_the_oracle(compressor):
    t = tensor_cases()["ids"].cuda(0)
    raw = t.cpu().numpy().tobytes()
    chunks = [raw[o:o + 65536] for o in range(0, len(raw), 65536)]
    ct = compressor.compress_tensor(t)
    want = oracle_blocks([planes.split(c, 4) for c in chunks], 65535)
    assert ct.offsets == [0] + list(np.cumsum([len(w) for w in want]))
    assert ct.blocks.cpu().numpy().tobytes() == b"".join(want)
    assert ct.nbytes < sum(len(b) for b in compressor.compress_batch(chunks, 65535))
