"""The ragged batch API on the GPU: many separate device buffers of different sizes, each compressed as
one LZ4 block on its own, and the reverse.  Expected bytes come from the oracle alone (oz_block per item,
oz_unlz4 per block), every comparison is byte-for-byte.  Run with -m gpu on an MI355X."""
import functools
from concurrent.futures import ThreadPoolExecutor

import pytest

from oracle import pyoracle
from smallz4_amd import _native, synth

pytestmark = pytest.mark.gpu
HDR = bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x70, 0xDF])
END = b"\0\0\0\0"

RAGGED = [0, 1, 5, 11, 12, 13, 16, 100, 4095, 4096, 4097, 65535, 65536, 65537, 70001, 200003, 0, 3]


def oracle_blocks(items, chain):
    # items are independent: the oracle runs them on threads (ctypes releases the GIL)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda x: pyoracle.oz_block(x, chain), items))


@functools.lru_cache(maxsize=None)
def ragged_case():
    """The ragged items as (offset, size) slices of one text: the k-th non-empty item starts at source
    alignment k mod 16, so the 16 of them cover every alignment."""
    slices, at, k = [], 0, 0
    for n in RAGGED:
        if n:
            at += (k - at) % 16
            k += 1
        slices.append((at, n))
        at += n
    text = synth.enwik8_like(at + 64, seed=41)
    return text, tuple(slices)


@functools.lru_cache(maxsize=None)
def ragged_expected(chain):
    text, slices = ragged_case()
    return tuple(oracle_blocks([text[a:a + n] for a, n in slices], chain))


def device_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


def check_parity(comp, items, chain):
    """compress_batch against the oracle, item by item; returns the expected blocks."""
    host = [x.cpu().numpy().tobytes() if hasattr(x, "cpu") else bytes(x) for x in items]
    want = oracle_blocks(host, chain)
    got = comp.compress_batch(items, chain)
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"item {i} ({len(host[i])} bytes) differs at chain {chain}"
    assert comp.last_block_sizes(len(items)) == [len(w) for w in want]
    return want


# ---- 1. ragged parity ------------------------------------------------------------------------
@pytest.mark.parametrize("chain", [0, 3, 6, 7, 65535])
def test_ragged_parity(compressor, chain):
    import torch
    text, slices = ragged_case()
    base = device_bytes(text)
    aligns = {(base.data_ptr() + a) % 16 for a, n in slices if n}
    assert aligns == set(range(16))
    sizes = [n for _, n in slices]
    ptrs = [base.data_ptr() + a if n else 0 for a, n in slices]
    cap = compressor.batch_bound(sizes)
    assert cap == sum(n + 4 for n in sizes)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    off = compressor.compress_batch_device(ptrs, sizes, out.data_ptr(), cap, chain)
    assert len(off) == len(sizes) + 1 and off[0] == 0
    assert all(off[i] <= off[i + 1] for i in range(len(sizes)))
    assert off[-1] <= cap
    raw = out[:off[-1]].cpu().numpy().tobytes()
    want = ragged_expected(chain)
    for i, n in enumerate(sizes):
        assert raw[off[i]:off[i + 1]] == want[i], f"item {i} ({n} bytes) differs at chain {chain}"
        if n == 0:
            assert off[i] == off[i + 1]
    assert compressor.last_block_sizes(len(sizes)) == [len(w) for w in want]


# ---- 2. content kinds in one batch -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def kinds():
    return (synth.random_bytes(70000, seed=1), bytes(70000), synth.runs(300000, seed=4, max_run=20000),
            synth.small_alphabet(300000, k=2, seed=2), synth.repeats(600000, seed=22, unit=30000, mutate_every=9000))


@pytest.mark.parametrize("chain", [7, 65535])
def test_content_kinds(compressor, chain):
    want = check_parity(compressor, list(kinds()), chain)
    assert want[0][:4] == bytes.fromhex("70110180")  # the random item is stored: word 0x80011170


# ---- 3. one large item among many small ------------------------------------------------------
def test_large_among_small(compressor):
    import random
    rng = random.Random(7)
    text = synth.enwik8_like((1 << 20) + 17 + 300 * 8192, seed=43)
    base = device_bytes(text)
    items, at = [], 0
    for k in range(301):
        n = (1 << 20) + 17 if k == 150 else rng.randrange(1024, 8193)
        items.append(base[at:at + n])
        at += n
    want = check_parity(compressor, items, 65535)
    # caller order: the large item's block sits between its neighbours', where its size says
    assert len(want[150]) > max(len(w) for i, w in enumerate(want) if i != 150)


# ---- 4. pieces -------------------------------------------------------------------------------
def test_pieces():
    import random
    import smallz4_amd
    rng = random.Random(11)
    sizes = [rng.randrange(16 << 10, 150 << 10) for _ in range(39)]
    sizes.insert(20, 2 << 20)  # larger than the piece: a piece on its own
    text = synth.enwik8_like(sum(sizes), seed=44)
    base = device_bytes(text)
    items, at = [], 0
    for n in sizes:
        items.append(base[at:at + n])
        at += n
    comp = smallz4_amd.Compressor(device=0)
    try:
        comp.set_batch_chunk(1 << 20)
        check_parity(comp, items, 65535)
    finally:
        comp.close()


def test_batch_buffers_are_accounted():
    """device_bytes / trim / set_device_limit cover the batch buffers (item table, mixed-piece staging, mover
    table, the decoder's extent table)."""
    import smallz4_amd
    text = synth.enwik8_like(400000, seed=51)
    items = [text[:3000], text[3000:203000], text[203000:230000], text[230000:]]  # LDS-sized and larger: a mixed piece
    limit = 1 << 30
    comp = smallz4_amd.Compressor(device=0)
    try:
        blocks = comp.compress_batch(items, 65535)
        assert comp.unlz4_batch(blocks) == items
        held = comp.device_bytes()
        assert held > sum(len(x) for x in items)
        comp.trim()
        assert comp.device_bytes() == 0
        comp.set_device_limit(limit)
        assert comp.compress_batch(items, 65535) == blocks
        assert comp.unlz4_batch(blocks) == items
        assert 0 < comp.device_bytes() <= limit
    finally:
        comp.close()


# ---- 5. identity with the uniform path -------------------------------------------------------
@pytest.mark.parametrize("chain", [3, 65535])
def test_identity_with_compress_blocks(compressor, chain):
    data = synth.enwik8_like(16 * 65536, seed=45)
    base = device_bytes(data)
    items = [base[k * 65536:(k + 1) * 65536] for k in range(16)]
    got = b"".join(compressor.compress_batch(items, chain))
    assert got == compressor.compress_blocks(base, 65536, chain, header="none")
    # and the uniform path still plans for itself after a ragged call
    head = data[:200000]
    assert compressor.compress_blocks(head, 65536, chain) == \
        HDR + b"".join(pyoracle.oz_block(head[o:o + 65536], chain) for o in range(0, 200000, 65536)) + END


# ---- 6. many tiny items ----------------------------------------------------------------------
def test_many_tiny_items(compressor):
    text = synth.enwik8_like(2000 * 64, seed=46)
    base = device_bytes(text)
    check_parity(compressor, [base[k * 64:(k + 1) * 64] for k in range(2000)], 65535)


# ---- 7. errors -------------------------------------------------------------------------------
def test_errors_leave_the_context_usable(compressor):
    import torch
    text = synth.enwik8_like(30000, seed=47)
    small = [text[:10000], text[10000:10007], text[10007:]]
    big = torch.zeros((4 << 20) + 1, dtype=torch.uint8, device="cuda:0")
    out = torch.empty((4 << 20) + 64, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(_native.NativeError, match=r"\(-1\)"):  # SZ4_E_ARG
        compressor.compress_batch_device([big.data_ptr()], [big.numel()], out.data_ptr(), out.numel(), 65535)
    check_parity(compressor, small, 65535)
    d = device_bytes(text)
    sizes = [10000, 20000]
    with pytest.raises(_native.NativeError, match=r"\(-3\)"):  # SZ4_E_CAPACITY
        compressor.compress_batch_device([d.data_ptr(), d.data_ptr() + 10000], sizes, out.data_ptr(),
                                         compressor.batch_bound(sizes) - 1, 65535)
    check_parity(compressor, small, 7)


# ---- 8. the decoder against the oracle's own blocks ------------------------------------------
@pytest.mark.parametrize("chain", [0, 65535])
def test_decoder_on_oracle_blocks(compressor, chain):
    text, slices = ragged_case()
    items = [text[a:a + n] for a, n in slices] + [kinds()[0]]
    blocks = list(ragged_expected(chain)) + [pyoracle.oz_block(kinds()[0], chain)]
    assert compressor.unlz4_batch(blocks) == items
    # query mode: the sizes alone
    offsets = [0]
    for b in blocks:
        offsets.append(offsets[-1] + len(b))
    d = device_bytes(b"".join(blocks))
    sizes = compressor.unlz4_batch_device(d.data_ptr(), offsets, 0, 0)
    want = [0]
    for x in items:
        want.append(want[-1] + len(x))
    assert sizes == want


# ---- 9. isolation ----------------------------------------------------------------------------
def test_items_do_not_see_each_other(compressor):
    text = synth.enwik8_like(1000, seed=48)
    item0 = pyoracle.oz_block(text, 65535)
    # 4 literals, a match of 4 at distance 8 (4 bytes below the item's first output byte), 5 literals
    payload = bytes([0x40]) + b"abcd" + bytes([0x08, 0x00, 0x50]) + b"vwxyz"
    item1 = len(payload).to_bytes(4, "little") + payload
    alone = b"abcd\0\0\0\0vwxyz"
    assert pyoracle.oz_unlz4(HDR + item1 + END) == alone
    assert compressor.unlz4_batch([item0, item1]) == [text, alone]
    # the dependent-frame reading of the same bytes is unchanged: the match reaches item 0's output
    linked = text + b"abcd" + text[-4:] + b"vwxyz"
    assert pyoracle.oz_unlz4(HDR + item0 + item1 + END) == linked
    assert compressor.unlz4(HDR + item0 + item1 + END) == linked


# ---- 10. corrupt -----------------------------------------------------------------------------
def test_corrupt_items(compressor):
    text = synth.enwik8_like(5000, seed=49)
    a, b = pyoracle.oz_block(text[:3000], 65535), pyoracle.oz_block(text[3000:], 65535)
    d = device_bytes(a + b)
    with pytest.raises(_native.NativeError, match=r"\(-6\)"):  # extent and size word disagree
        compressor.unlz4_batch_device(d.data_ptr(), [0, len(a) + 1, len(a) + len(b)], 0, 0)
    assert compressor.unlz4_batch([a, b]) == [text[:3000], text[3000:]]
    with pytest.raises(_native.NativeError, match=r"\(-6\)"):  # shorter than a size word, but not empty
        compressor.unlz4_batch_device(d.data_ptr(), [0, 3], 0, 0)
    assert compressor.unlz4_batch([b, b"", a]) == [text[3000:], b"", text[:3000]]


# ---- 11. a large decoded item ----------------------------------------------------------------
def test_large_item_round_trip(compressor):
    text = synth.enwik8_like(1 << 20, seed=50)
    blocks = compressor.compress_batch([text, b"", text[:77]], 65535)
    assert len(blocks[0]) - 4 >= 256 << 10  # its payload is in the range the frame decoder would split
    assert blocks[1] == b""
    assert compressor.unlz4_batch(blocks) == [text, b"", text[:77]]
