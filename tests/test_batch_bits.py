"""The bit-plane shuffle of the filtered batch API on the GPU: a BITS item is shuffled into its bit rows while it
is staged and unshuffled after the batch decoder.  Expected bytes come only from the oracle on the host model
(oz_block(planes.bit_split(item, E)), and planes.split for the BYTES items beside them) and from the items
themselves; every comparison is byte for byte.  Run with -m gpu on an MI355X."""
import ctypes
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import _native, planes, synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8)
BYTES, BITS = _native.SZ4_FILTER_BYTES, _native.SZ4_FILTER_BITS
CHAINS = (0, 3, 7, 65535)


def sizes_for(E):
    """g = 0, the first row byte, the first whole 16-byte row word (128 elements), rows that do not start at a
    multiple of 16, left-over elements with and without a tail, items of both finder kinds."""
    return [0, 1, E - 1, 8 * E - 1, 8 * E, 8 * E + 1, 16 * E, 127 * E, 128 * E, 128 * E + 1, 129 * E + 3, 1024 * E,
            1032 * E + 1, 4097, 65536, 65537, 70001]


def oracle_blocks(items, chain):
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda x: pyoracle.oz_block(x, chain), items))


def filtered(item, E, f):
    return planes.bit_split(item, E) if f == BITS else planes.split(item, E)


@functools.lru_cache(maxsize=None)
def payload(E):
    """What items of width E hold: text at width 1, weights drawn from normal(0, 0.02) as bf16, fp32 and fp64 at
    the others (counters would make constant bit rows that join into runs the oracle is quadratic in)."""
    if E == 1:
        return synth.enwik8_like(160_000, seed=81)
    w = np.random.default_rng(80 + E).normal(0, 0.02, 160_000 // E + 8)
    if E == 2:
        return (w.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes()
    return w.astype(np.float32 if E == 4 else np.float64).tobytes()


@functools.lru_cache(maxsize=None)
def bits_case():
    """(buffer, ((offset, size, E, filter), ...)): every size of every width twice, BITS then BYTES, cut from one
    buffer so that the k-th non-empty item of a filter starts at source alignment k mod 16 (k + 5 for BYTES);
    then a random (stored) and an all-zero BITS item."""
    spec = [(n, E, f) for E in WIDTHS for n in sizes_for(E) for f in (BITS, BYTES)] + [(5000, 4, BITS), (5000, 2, BITS)]
    buf, slices, k, used = bytearray(), [], {BITS: 0, BYTES: 5}, {E: 0 for E in WIDTHS}
    for n, E, f in spec:
        if n:
            buf += bytes((k[f] - len(buf)) % 16)
            k[f] += 1
        slices.append((len(buf), n, E, f))
        if f == BITS:  # the BYTES twin holds the same bytes
            used[E] = (used[E] + 4 * n) % 80_000
        buf += payload(E)[used[E]:used[E] + n]
    a, n, _, _ = slices[-2]
    buf[a:a + n] = synth.random_bytes(n, seed=83)
    a, n, _, _ = slices[-1]
    buf[a:a + n] = bytes(n)
    return bytes(buf) + bytes(64), tuple(slices)


def case_items():
    buf, slices = bits_case()
    return [buf[a:a + n] for a, n, _, _ in slices]


@functools.lru_cache(maxsize=None)
def case_filtered():
    return tuple(filtered(x, E, f) for x, (_, _, E, f) in zip(case_items(), bits_case()[1]))


@functools.lru_cache(maxsize=None)
def case_expected(chain):
    return tuple(oracle_blocks(list(case_filtered()), chain))


def device_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


_gpu_blocks = {}


def gpu_case(comp, chain):
    """The case compressed by the filtered call: (raw bytes, offsets, reported sizes), once per chain."""
    if chain not in _gpu_blocks:
        import torch
        buf, slices = bits_case()
        base = device_bytes(buf)
        for f in (BITS, BYTES):
            assert {(base.data_ptr() + a) % 16 for a, n, _, g in slices if n and g == f} == set(range(16))
        sizes = [n for _, n, _, _ in slices]
        ptrs = [base.data_ptr() + a if n else 0 for a, n, _, _ in slices]
        cap = comp.batch_bound(sizes)
        out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
        off = comp.compress_batch_filtered_device(ptrs, sizes, [E for _, _, E, _ in slices], [f for _, _, _, f in slices],
                                                  out.data_ptr(), cap, chain)
        _gpu_blocks[chain] = (out[:off[-1]].cpu().numpy().tobytes(), off, comp.last_block_sizes(len(sizes)))
    return _gpu_blocks[chain]


# ---- 1. parity -------------------------------------------------------------------------------
@pytest.mark.parametrize("chain", CHAINS)
def test_bits_parity(compressor, chain):
    _, slices = bits_case()
    raw, off, reported = gpu_case(compressor, chain)
    want = case_expected(chain)
    assert len(off) == len(slices) + 1 and off[0] == 0
    if chain == 0:  # a stored block is the size word and the filtered bytes: the gather alone
        for i, s in enumerate(case_filtered()):
            assert raw[off[i]:off[i + 1]] == ((len(s) | 0x80000000).to_bytes(4, "little") + s if s else b""), \
                f"item {i} {slices[i][1:]} is not staged as its filter says"
    for i, (a, n, E, f) in enumerate(slices):
        assert raw[off[i]:off[i + 1]] == want[i], f"item {i} ({n} bytes, width {E}, filter {f}) differs at chain {chain}"
    assert reported == [len(w) for w in want]


# ---- 2. one large item, for the HBM finder -------------------------------------------------------
def test_large_bits_item(compressor):
    item = synth.enwik8_like(200003, seed=84)
    blocks = compressor.compress_batch_typed([item], [4], 65535, filters="bits")
    assert blocks[0] == pyoracle.oz_block(planes.bit_split(item, 4), 65535)
    assert compressor.unlz4_batch_typed(blocks, [4], "bits") == [item]


# ---- 3. round trip ---------------------------------------------------------------------------
def round_trip_order(order):
    """The case's items in case order, or with the items whose size is a multiple of 64 first: from an aligned
    d_out those all land where the unshuffle takes whole units."""
    slices = bits_case()[1]
    idx = list(range(len(slices)))
    if order == "multiples of 64 first":
        idx.sort(key=lambda i: (slices[i][1] % 64 != 0, i))
    return idx


@pytest.mark.parametrize("order", ["case", "multiples of 64 first"])
@pytest.mark.parametrize("lead", [33, 64])  # d_out at an odd address, and at an aligned one
def test_round_trip(compressor, lead, order):
    import torch
    idx = round_trip_order(order)
    slices = bits_case()[1]
    items = [case_items()[i] for i in idx]
    elems = [slices[i][2] for i in idx]
    filters = [slices[i][3] for i in idx]
    raw, coff, _ = gpu_case(compressor, 7)
    blocks = [raw[coff[i]:coff[i + 1]] for i in idx]
    off = [0]
    for b in blocks:
        off.append(off[-1] + len(b))
    d = device_bytes(b"".join(blocks))
    want_off = [0]
    for x in items:
        want_off.append(want_off[-1] + len(x))
    total = want_off[-1]
    assert compressor.unlz4_batch_filtered_device(d.data_ptr(), off, elems, filters, 0, 0) == want_off  # query mode
    buf = torch.full((lead + total + 64,), 0xA5, dtype=torch.uint8, device="cuda:0")
    d_out = buf.data_ptr() + lead
    assert d_out % 16 == lead % 16
    # one byte short: SZ4_E_CAPACITY, the offsets filled in, nothing written
    o = (ctypes.c_uint64 * len(off))(*off)
    w = (ctypes.c_uint8 * len(elems))(*elems)
    f = (ctypes.c_uint8 * len(elems))(*filters)
    res = (ctypes.c_uint64 * len(off))()
    rc = compressor._lib.sz4_unlz4_batch_filtered_device(compressor._h, ctypes.c_void_p(d.data_ptr()), o, w, f, len(elems),
                                                         ctypes.c_void_p(d_out), total - 1, res, None)
    assert rc == _native.SZ4_E_CAPACITY
    assert list(res) == want_off
    assert bool((buf == 0xA5).all())
    assert compressor.unlz4_batch_filtered_device(d.data_ptr(), off, elems, filters, d_out, total) == want_off
    host = buf.cpu().numpy().tobytes()
    assert host[:lead] == b"\xA5" * lead and host[lead + total:] == b"\xA5" * 64
    for i, x in enumerate(items):
        assert host[lead + want_off[i]:lead + want_off[i + 1]] == x, \
            f"item {i} ({len(x)} bytes, width {elems[i]}, filter {filters[i]})"
    names = ["bits" if g == BITS else "bytes" for g in filters]
    assert compressor.unlz4_batch_typed(blocks, elems, names) == items


# ---- 4. filtered blocks are ordinary blocks ------------------------------------------------------
def test_bits_blocks_decode_to_the_shuffle(compressor):
    raw, off, _ = gpu_case(compressor, 3)
    blocks = [raw[off[i]:off[i + 1]] for i in range(len(off) - 1)]
    assert compressor.unlz4_batch(blocks) == list(case_filtered())


# ---- 5. no filters, or BYTES throughout, is the typed call ---------------------------------------
def test_bytes_filter_is_the_typed_call(compressor):
    import torch
    import test_batch_typed as typed
    buf, slices = typed.typed_case()
    base = device_bytes(buf)
    sizes = [n for _, n, _ in slices]
    ptrs = [base.data_ptr() + a if n else 0 for a, n, _ in slices]
    elems = [E for _, _, E in slices]
    cap = compressor.batch_bound(sizes)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    off = compressor.compress_batch_typed_device(ptrs, sizes, elems, out.data_ptr(), cap, 7)
    want = out[:off[-1]].cpu().numpy().tobytes()
    for filters in (None, [BYTES] * len(sizes)):
        out.zero_()
        assert compressor.compress_batch_filtered_device(ptrs, sizes, elems, filters, out.data_ptr(), cap, 7) == off
        assert out[:off[-1]].cpu().numpy().tobytes() == want
    d = device_bytes(want)
    total = sum(sizes)
    dec = torch.empty(total + 16, dtype=torch.uint8, device="cuda:0")
    want_off = compressor.unlz4_batch_typed_device(d.data_ptr(), off, elems, dec.data_ptr(), total)
    items = dec[:total].cpu().numpy().tobytes()
    assert items == b"".join(buf[a:a + n] for a, n, _ in slices)
    for filters in (None, [BYTES] * len(sizes)):
        dec.zero_()
        assert compressor.unlz4_batch_filtered_device(d.data_ptr(), off, elems, filters, dec.data_ptr(), total) == want_off
        assert dec[:total].cpu().numpy().tobytes() == items


# ---- 6. widths of 1 throughout with one BITS item is not the plain call ------------------------------
def test_width_one_with_one_bits_item(compressor):
    import torch
    text = synth.enwik8_like(30_000, seed=85)
    cuts = [0, 1000, 1003, 9195, 9195, 20_000, 30_000]  # item 2 (8192 bytes at an odd address) is the BITS one
    base = device_bytes(text)
    sizes = [b - a for a, b in zip(cuts, cuts[1:])]
    ptrs = [base.data_ptr() + a if n else 0 for a, n in zip(cuts, sizes)]
    filters = [BYTES] * len(sizes)
    filters[2] = BITS
    cap = compressor.batch_bound(sizes)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    off = compressor.compress_batch_device(ptrs, sizes, out.data_ptr(), cap, 7)
    raw = out[:off[-1]].cpu().numpy().tobytes()
    plain = [raw[off[i]:off[i + 1]] for i in range(len(sizes))]
    out.zero_()
    off = compressor.compress_batch_filtered_device(ptrs, sizes, [1] * len(sizes), filters, out.data_ptr(), cap, 7)
    raw = out[:off[-1]].cpu().numpy().tobytes()
    got = [raw[off[i]:off[i + 1]] for i in range(len(sizes))]
    assert [i for i in range(len(sizes)) if got[i] != plain[i]] == [2]
    assert got[2] == pyoracle.oz_block(planes.bit_split(text[cuts[2]:cuts[3]], 1), 7)
    names = ["bits" if f == BITS else "bytes" for f in filters]
    assert compressor.unlz4_batch_typed(got, [1] * len(sizes), names) == [text[a:b] for a, b in zip(cuts, cuts[1:])]


# ---- 7. errors -------------------------------------------------------------------------------
@pytest.mark.parametrize("elem,filt", [(4, 2), (3, 1)])
def test_bad_filter_or_width_is_refused(compressor, elem, filt):
    import torch
    d = device_bytes(synth.enwik8_like(3000, seed=86))
    out = torch.full((4000,), 0xA5, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):  # SZ4_E_ARG
        compressor.compress_batch_filtered_device([d.data_ptr(), d.data_ptr() + 1000], [1000, 2000], [4, elem], [BITS, filt],
                                                  out.data_ptr(), 4000, 7)
    assert bool((out == 0xA5).all())
    block = pyoracle.oz_block(planes.bit_split(bytes(1000), 4), 7)
    b = device_bytes(block)
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):
        compressor.unlz4_batch_filtered_device(b.data_ptr(), [0, len(block)], [elem], [filt], out.data_ptr(), 4000)
    assert bool((out == 0xA5).all())
    with pytest.raises(ValueError):
        compressor.compress_batch_typed([b"abcdefgh"], [4], filters="nibbles")
    assert compressor.unlz4_batch_typed([block], [4], "bits") == [bytes(1000)]


# ---- 8. several pieces -----------------------------------------------------------------------
def test_pieces_give_the_same_bytes(compressor):
    import smallz4_amd
    items = case_items()
    slices = bits_case()[1]
    elems = [E for _, _, E, _ in slices]
    names = ["bits" if f == BITS else "bytes" for _, _, _, f in slices]
    raw, off, _ = gpu_case(compressor, 7)
    one = [raw[off[i]:off[i + 1]] for i in range(len(items))]
    # the case is 1.2 MB of staged bytes: at the smallest piece size it runs as two pieces at least
    assert sum(len(x) for x in items) > 1 << 20
    comp = smallz4_amd.Compressor(device=0)
    try:
        comp.set_batch_chunk(1 << 20)
        assert comp.compress_batch_typed(items, elems, 7, names) == one
    finally:
        comp.close()


# ---- 9. tensors ------------------------------------------------------------------------------
def tensor_case(name):
    import torch
    import test_batch_typed as typed
    if name == "fp16":
        return torch.from_numpy(np.random.default_rng(70).normal(0, 0.02, 200_000).astype(np.float16))
    return typed.tensor_cases()[name]


@pytest.mark.parametrize("name", ["bf16", "fp32", "uint8", "view", "empty", "fp16", "stamps"])
def test_tensor_round_trip(compressor, name):
    import torch
    t = tensor_case(name).cuda(0)
    ct = compressor.compress_tensor(t, filter="bits")
    assert ct.filter == "bits" and ct.blocks.numel() == ct.offsets[-1]
    assert ct.dtype == t.dtype and ct.shape == tuple(t.shape) and ct.chunk_bytes == 65536
    back = compressor.decompress_tensor(ct)
    assert back.is_cuda and back.dtype == t.dtype and back.shape == t.shape
    same = back.contiguous().reshape(-1).view(torch.uint8) == t.contiguous().reshape(-1).view(torch.uint8)
    assert bool(same.all())
    if name == "fp16":  # what the filter is for: fp16 weights gain nothing from the byte split
        plain = compressor.compress_tensor(t)
        assert plain.filter == "bytes" and ct.nbytes < plain.nbytes
        raw = t.cpu().numpy().tobytes()
        assert ct.blocks[:ct.offsets[1]].cpu().numpy().tobytes() == pyoracle.oz_block(planes.bit_split(raw[:65536], 2), 65535)


def test_decode_queue_refuses_a_bits_tensor(compressor):
    import torch
    t = tensor_case("fp32").cuda(0)
    ct = compressor.compress_tensor(t, filter="bits")
    q = compressor.decode_queue(16, 1 << 20)
    try:
        with pytest.raises(ValueError):
            q.tensor_tables(ct, torch.empty_like(t))
        q.tensor_tables(compressor.compress_tensor(t), torch.empty_like(t))  # the byte filter still passes
    finally:
        q.close()
