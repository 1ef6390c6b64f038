"""The compress queue (sz4_cq_*, Compressor.compress_queue) on the GPU: a device table of source pointers in,
the blocks back to back in one output buffer and device tables of their addresses, sizes and statuses out,
nothing on the host in between.  Expected bytes come only from the oracle on the host model's split
(oz_block(planes.split(item, E), chain)); every comparison is byte-for-byte.  Inputs are built as
tests/test_batch_typed.py builds its own: text, then increasing counters, one random and one all-zero item,
all slices of one device buffer so that the non-empty items cover source alignments 0 .. 15.
Run with -m gpu on an MI355X."""
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import CompressedTensor, _native, planes, synth

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 4, 8)
CHAINS = (0, 7, 16, 65535)
SENTINEL = 0xA5
OK, ARG = _native.SZ4_ITEM_OK, _native.SZ4_ITEM_ARG
LDS_MAX = 65541  # the largest item whose window fits the finders' LDS (65552 bytes hold the item and 8 more, in whole words)


@pytest.fixture(scope="module")
def compressor(compressor):
    """The session's fixture decides whether there is a GPU; the tests here run on a context of their own."""
    import smallz4_amd
    c = smallz4_amd.Compressor(device=0)
    yield c
    c.close()


def sizes_for(E):
    return [0, 1, E - 1, E, E + 1, 15, 16, 17, 16 * E - 1, 16 * E, 16 * E + 1, 255, 256, 257, 1000, 4095, 4096, 4097,
            65535, 65536, LDS_MAX]


SETS = {
    # the last two items of `small` are overwritten: one random (stored), one all zero
    "small": [(n, E) for E in WIDTHS for n in sizes_for(E)] + [(5000, 4), (5000, 2)],
    "large": [(LDS_MAX + 1, 1), (70001, 4), (200003, 8)],
    "mixed": [(1000, 1), (LDS_MAX, 1), (LDS_MAX + 1, 1), (70001, 1)],
}


def numeric_bytes(n, seed):
    """Increasing int32 counters, then increasing int64 ones (tests/test_batch_typed.py)."""
    rng = np.random.default_rng(seed)
    a = (np.cumsum(rng.integers(0, 70000, n // 8 + 8)) & 0x7FFFFFFF).astype(np.int32).tobytes()
    b = np.cumsum(rng.integers(0, 2 ** 44, n // 16 + 8, dtype=np.int64)).astype(np.int64).tobytes()
    return (a + b)[:n]


@functools.lru_cache(maxsize=None)
def case(name):
    """(buffer, ((offset, size, E), ...)): the k-th non-empty item starts at source alignment k mod 16."""
    slices, at, k = [], 0, 0
    for n, E in SETS[name]:
        if n:
            at += (k - at) % 16
            k += 1
        slices.append((at, n, E))
        at += n
    half = at // 2
    buf = bytearray(synth.enwik8_like(half, seed=71) + numeric_bytes(at + 64 - half, seed=72))
    if name == "small":
        a, n, _ = slices[-2]
        buf[a:a + n] = synth.random_bytes(n, seed=73)
        a, n, _ = slices[-1]
        buf[a:a + n] = bytes(n)
    return bytes(buf), tuple(slices)


def oracle_blocks(items, elems, chain):
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda p: pyoracle.oz_block(planes.split(p[0], p[1]), chain) if p[0] else b"", zip(items, elems)))


@functools.lru_cache(maxsize=None)
def expected(name, chain):
    buf, slices = case(name)
    return tuple(oracle_blocks([buf[a:a + n] for a, n, _ in slices], [E for _, _, E in slices], chain))


def device_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


class Tables:
    """The device tables of one queue and its output: `bound` bytes, `lead` bytes into a larger tensor of 0xA5."""

    def __init__(self, q, lead=3, tail=256):
        import torch
        dev = "cuda:0"
        self.q, self.lead = q, lead
        self.whole = torch.full((lead + q.bound + tail,), SENTINEL, dtype=torch.uint8, device=dev)
        self.out = self.whole[lead:lead + q.bound]
        self.src = torch.zeros(q.count, dtype=torch.int64, device=dev)
        self.ptrs = torch.full((q.count,), -7, dtype=torch.int64, device=dev)
        self.sizes = torch.full((q.count,), -7, dtype=torch.int32, device=dev)
        self.status = torch.full((q.count,), -7, dtype=torch.int32, device=dev)
        self.total = torch.full((1,), -7, dtype=torch.int64, device=dev)

    def set_sources(self, ptrs):
        import torch
        self.src.copy_(torch.tensor(list(ptrs), dtype=torch.int64))

    def enqueue(self):
        self.q.enqueue(self.src, self.out, self.ptrs, self.sizes, self.status, self.total)

    def check(self, want, statuses=None, what=""):
        """Blocks `want` back to back from the start of out, tables to match, and no byte outside out written."""
        import torch
        torch.cuda.synchronize()
        host = self.whole.cpu().numpy().tobytes()
        lead, bound = self.lead, self.q.bound
        base = self.out.data_ptr()
        at, ptrs = 0, []
        for w in want:
            ptrs.append(base + at)
            at += len(w)
        assert self.total.cpu().tolist() == [at], f"{what}: total"
        assert self.sizes.cpu().tolist() == [len(w) for w in want], f"{what}: block sizes"
        assert self.status.cpu().tolist() == (statuses or [OK] * len(want)), f"{what}: statuses"
        got = self.ptrs.cpu().tolist()
        assert got == ptrs, f"{what}: block addresses"
        at = 0
        for i, w in enumerate(want):
            g = host[lead + at:lead + at + len(w)]
            if g != w:
                k = next(j for j in range(len(w)) if g[j] != w[j])
                pytest.fail(f"{what}: item {i} ({len(w)} block bytes) differs at offset {k}: {g[k:k + 8].hex()} for {w[k:k + 8].hex()}")
            at += len(w)
        assert host[:lead] == bytes([SENTINEL]) * lead, f"{what}: bytes before the output were written"
        assert host[lead + bound:] == bytes([SENTINEL]) * (len(host) - lead - bound), f"{what}: bytes at or beyond the bound were written"


def queue_for(comp, name, chain):
    _, slices = case(name)
    return comp.compress_queue([n for _, n, _ in slices], [E for _, _, E in slices], chain)


def sources(base, slices):
    # an empty item's entry is never looked at: garbage
    return [base.data_ptr() + a if n else 0x5A5A5A5A5A5A for a, n, _ in slices]


# ---- 1. parity -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SETS))
@pytest.mark.parametrize("chain", CHAINS)
def test_parity(compressor, chain, name):
    buf, slices = case(name)
    base = device_bytes(buf)
    if name == "small":
        assert {(base.data_ptr() + a) % 16 for a, n, _ in slices if n} == set(range(16))
    q = queue_for(compressor, name, chain)
    try:
        sizes = [n for _, n, _ in slices]
        assert q.count == len(slices) and q.bound == compressor.batch_bound(sizes) == sum(n + 4 for n in sizes)
        t = Tables(q)
        t.set_sources(sources(base, slices))
        t.enqueue()
        want = expected(name, chain)
        t.check(want, what=f"{name} at chain {chain}")
        if chain == 0:  # a stored block is the size word and the split bytes
            for (a, n, E), w in zip(slices, want):
                s = planes.split(buf[a:a + n], E)
                assert w == ((len(s) | 0x80000000).to_bytes(4, "little") + s if s else b"")
    finally:
        q.close()


@pytest.mark.parametrize("chain", [0, 65535])
def test_one_item_and_empty_queues(compressor, chain):
    data = synth.enwik8_like(3001, seed=74)
    base = device_bytes(bytes(5) + data)
    q = compressor.compress_queue([len(data)], None, chain)
    try:
        t = Tables(q)
        t.set_sources([base.data_ptr() + 5])
        t.enqueue()
        t.check([pyoracle.oz_block(data, chain)], what="one item")
    finally:
        q.close()
    q = compressor.compress_queue([0, 0, 0], [1, 4, 8], chain)
    try:
        assert q.bound == 12
        t = Tables(q)
        t.set_sources([0x5A5A5A5A5A5A, 1, -1])
        t.enqueue()
        t.check([b"", b"", b""], what="three empty items")
    finally:
        q.close()


# ---- 2. identity with the synchronous call ---------------------------------------------------
@pytest.mark.parametrize("name,chain", [("small", 7), ("mixed", 65535)])
def test_identity_with_the_synchronous_call(compressor, name, chain):
    import torch
    buf, slices = case(name)
    base = device_bytes(buf)
    sizes = [n for _, n, _ in slices]
    elems = [E for _, _, E in slices]
    cap = compressor.batch_bound(sizes)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    off = compressor.compress_batch_typed_device([base.data_ptr() + a if n else 0 for a, n, _ in slices], sizes, elems,
                                                 out.data_ptr(), cap, chain)
    raw = out[:off[-1]].cpu().numpy().tobytes()
    q = queue_for(compressor, name, chain)
    try:
        t = Tables(q)
        t.set_sources(sources(base, slices))
        t.enqueue()
        t.check([raw[off[i]:off[i + 1]] for i in range(len(sizes))], what="against compress_batch_typed_device")
        assert [p - t.out.data_ptr() for p in t.ptrs.cpu().tolist()] == off[:-1]
    finally:
        q.close()


# ---- 3. bounds of the output -----------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 16])
def test_nothing_is_written_at_or_beyond_the_bound(compressor, lead):
    """out is exactly `bound` long inside a larger buffer of 0xA5, at three alignments; the random item is stored,
    so its block fills its share of the bound to the last byte."""
    data = synth.random_bytes(70001, seed=75)
    base = device_bytes(data)
    q = compressor.compress_queue([70001, 0, 13], [1, 2, 4], 65535)
    try:
        t = Tables(q, lead=lead)
        assert t.out.numel() == q.bound
        t.set_sources([base.data_ptr(), 0, base.data_ptr() + 100])
        t.enqueue()
        want = [pyoracle.oz_block(data, 65535), b"", pyoracle.oz_block(planes.split(data[100:113], 4), 65535)]
        assert sum(len(w) for w in want) == q.bound - 4  # stored blocks: only the empty item's word is unused
        t.check(want, what=f"output {lead} bytes into its buffer")
    finally:
        q.close()


# ---- 4. the queue's scratch is its own -------------------------------------------------------
def test_other_calls_between_enqueues(compressor):
    buf, slices = case("mixed")
    base = device_bytes(buf)
    q = queue_for(compressor, "mixed", 65535)
    try:
        t = Tables(q)
        t.set_sources(sources(base, slices))
        want = expected("mixed", 65535)
        t.enqueue()
        t.check(want, what="first enqueue")
        items = [buf[a:a + n] for a, n, _ in slices]
        assert compressor.compress_batch(items, 3) == [pyoracle.oz_block(x, 3) for x in items]
        frame = compressor.compress_blocks(buf[:150_000], 32768, 65535)
        assert pyoracle.oz_unlz4(frame) == buf[:150_000]
        t.whole.fill_(SENTINEL)
        t.ptrs.fill_(-7), t.sizes.fill_(-7), t.status.fill_(-7), t.total.fill_(-7)
        t.enqueue()
        t.check(want, what="enqueue after other calls on the context")
    finally:
        q.close()


# ---- 5. graph capture ------------------------------------------------------------------------
def test_captured_enqueue_replays_on_rewritten_tables(compressor):
    """One enqueue of a 64-item queue captured on torch's capture stream and replayed three times, each time
    over a pointer table rewritten to other slices.  A synchronisation or an allocation inside the enqueue
    would fail the capture with a HIP error."""
    import torch
    count = 64
    sizes = [4096 + (k * 977) % 61441 for k in range(count)]
    sizes[0], sizes[-1] = 4096, 65536
    elems = [WIDTHS[k % 4] for k in range(count)]
    assert min(sizes) == 4096 and max(sizes) == 65536
    data = synth.enwik8_like(3 << 20, seed=76) + numeric_bytes(1 << 20, seed=77)
    base = device_bytes(data)
    q = compressor.compress_queue(sizes, elems, 65535)
    try:
        t = Tables(q)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t.enqueue()
        for rep in range(3):
            offs = [((rep * 64 + k) * 48611 + 7 * rep + k) % (len(data) - 65536) for k in range(count)]
            t.set_sources([base.data_ptr() + o for o in offs])
            t.whole.fill_(SENTINEL)
            t.ptrs.fill_(-7), t.sizes.fill_(-7), t.status.fill_(-7), t.total.fill_(-7)
            g.replay()
            want = oracle_blocks([data[o:o + n] for o, n in zip(offs, sizes)], elems, 65535)
            t.check(want, what=f"replay {rep}")
        del g
    finally:
        q.close()


@pytest.mark.parametrize("count", [1, 8])
def test_captured_enqueue_replays_alike(compressor, count):
    """Every replay of one captured enqueue gives the first one's result, with the output zeroed (a memset on
    the stream) and the result tables read back to the host between the replays.  An enqueue that cleared its
    status word with a captured memset reported SZ4_ITEM_INTERNAL from the second replay on in exactly this
    sequence: the enqueue stores its clears from kernels."""
    import torch
    n = 65536
    data = synth.enwik8_like(n * count, seed=82)
    base = device_bytes(data)
    want = oracle_blocks([data[k * n:(k + 1) * n] for k in range(count)], [1] * count, 65535)
    q = compressor.compress_queue([n] * count, None, 65535)
    try:
        t = Tables(q)
        t.set_sources([base.data_ptr() + k * n for k in range(count)])
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t.enqueue()
        for rep in range(4):
            t.whole.zero_()
            t.whole[:t.lead].fill_(SENTINEL), t.whole[t.lead + q.bound:].fill_(SENTINEL)
            t.status.fill_(-1), t.total.fill_(-1)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert t.status.cpu().tolist() == [OK] * count and int(t.total[0]) == sum(len(w) for w in want), f"replay {rep}"
            t.check(want, what=f"replay {rep}")
        del g
    finally:
        q.close()


# ---- 6. round trip in one graph --------------------------------------------------------------
def test_round_trip_in_one_graph(compressor):
    """cq.enqueue -> dq.enqueue wired through block_ptrs / block_sizes in one captured graph: a bf16 tensor in
    64 KiB chunks comes back equal, twice, with the tensor rewritten in place between the replays."""
    import torch
    rng = np.random.default_rng(78)

    def fresh():
        return torch.from_numpy(rng.normal(0, 0.02, 100_003).astype(np.float32)).to(torch.bfloat16).cuda(0)

    t = fresh()
    chunk = 65536
    nbytes = t.numel() * 2
    sizes = [min(chunk, nbytes - o) for o in range(0, nbytes, chunk)]
    count = len(sizes)
    assert count == 4 and sizes[-1] < chunk
    cq = compressor.compress_queue(sizes, [2] * count, 65535)
    dq = compressor.decode_queue(count, cq.bound)
    try:
        c = Tables(cq)
        c.src = cq.tensor_tables(t)
        assert c.src.cpu().tolist() == [t.data_ptr() + k * chunk for k in range(count)]
        back = torch.zeros_like(t)
        # the decode side's destination tables: dq.tensor_tables over the output buffer cut at its worst-case offsets
        worst = [0]
        for n in sizes:
            worst.append(worst[-1] + n + 4)
        d = dq.tensor_tables(CompressedTensor(c.out, worst, t.dtype, tuple(t.shape), chunk), back)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.enqueue()
            dq.enqueue(c.ptrs, c.sizes, d.dst_ptrs, d.dst_caps, d.out_sizes, d.status, elems=d.elems, count=count)
        for rep in range(2):
            if rep:
                t.copy_(fresh())
            back.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert c.status.cpu().tolist() == [OK] * count and d.status.cpu().tolist() == [OK] * count, f"replay {rep}"
            assert d.out_sizes.cpu().tolist() == sizes
            assert bool((back.view(torch.uint8) == t.view(torch.uint8)).all()), f"replay {rep}"
            raw = t.view(torch.uint8).cpu().numpy().tobytes()
            c.check(oracle_blocks([raw[o:o + chunk] for o in range(0, nbytes, chunk)], [2] * count, 65535), what=f"replay {rep}")
        del g
    finally:
        dq.close()
        cq.close()


# ---- 7. errors -------------------------------------------------------------------------------
def test_create_refuses(compressor):
    bad = [([], None, 65535), ([16] * 32769, None, 65535), ([100, (4 << 20) + 1], None, 65535), ([100, 100], [1, 3], 65535),
           ([100], None, 3)]
    for sizes, elems, chain in bad:
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            compressor.compress_queue(sizes, elems, chain)
    for chain in (1, 6, 65536):
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            compressor.compress_queue([100], None, chain)
    compressor.compress_queue([100, 4 << 20], [8, 1], 7).close()  # the limits themselves are accepted
    compressor.compress_queue([16] * 32768, None, 0).close()


def test_short_output_is_refused_before_any_work(compressor):
    import torch
    data = synth.enwik8_like(5000, seed=79)
    base = device_bytes(data)
    q = compressor.compress_queue([3000, 2000], None, 65535)
    try:
        t = Tables(q)
        t.set_sources([base.data_ptr(), base.data_ptr() + 3000])
        t.out = t.whole[t.lead:t.lead + q.bound - 1]
        with pytest.raises(_native.NativeError, match=r"\(-3\)"):
            t.enqueue()
        torch.cuda.synchronize()
        assert bool((t.whole == SENTINEL).all())
        assert t.ptrs.cpu().tolist() == [-7, -7] and t.sizes.cpu().tolist() == [-7, -7]
        assert t.status.cpu().tolist() == [-7, -7] and t.total.cpu().tolist() == [-7]
    finally:
        q.close()


def test_null_source_fails_alone(compressor):
    """A null table entry of a non-empty item is never dereferenced: the item is compressed as zeros and gets
    SZ4_ITEM_ARG, every other item its oracle bytes.  (An entry the kernel must skip; nothing here faults.)"""
    data = synth.enwik8_like(9000, seed=80)
    base = device_bytes(data)
    for elems in (None, [1, 4, 2, 1]):
        q = compressor.compress_queue([3000, 1000, 0, 5000], elems, 65535)
        try:
            t = Tables(q)
            t.set_sources([base.data_ptr() + 1, 0, 0, base.data_ptr() + 3001])
            t.enqueue()
            e = elems or [1] * 4
            want = [pyoracle.oz_block(planes.split(data[1:3001], e[0]), 65535), pyoracle.oz_block(bytes(1000), 65535), b"",
                    pyoracle.oz_block(planes.split(data[3001:8001], e[3]), 65535)]
            t.check(want, statuses=[OK, ARG, OK, OK], what=f"widths {elems}")
        finally:
            q.close()


# ---- 8. limits and lifetime ------------------------------------------------------------------
def test_limits_and_lifetime(compressor):
    """A context of its own, so that its device bytes are the queue's and this test's alone."""
    import smallz4_amd
    comp = smallz4_amd.Compressor(device=0)
    q = None
    try:
        assert comp.device_bytes() == 0
        n, count = 65536, 8
        data = synth.enwik8_like(n * count, seed=81)
        base = device_bytes(data)
        want = oracle_blocks([data[k * n:(k + 1) * n] for k in range(count)], [1] * count, 65535)
        q = comp.compress_queue([n] * count, None, 65535)
        held = comp.device_bytes()
        assert held >= 36 * n * count  # the staged bytes: every size is a multiple of 64
        t = Tables(q)
        t.set_sources([base.data_ptr() + k * n for k in range(count)])

        def compresses(what):
            t.whole.fill_(SENTINEL)
            t.enqueue()
            t.check(want, what=what)

        compresses("after create")
        # trim leaves the queue's scratch, and only that
        comp.compress_batch([data[:5000], data[5000:70000]], 3)
        assert comp.device_bytes() > held
        comp.trim()
        assert comp.device_bytes() == held
        compresses("after trim")
        # a second queue over the bound leaves nothing allocated, and the first where it was
        comp.set_device_limit(comp.device_bytes())
        with pytest.raises(_native.NativeError, match=r"\(-4\)"):
            comp.compress_queue([n] * count, None, 65535)
        assert comp.device_bytes() == held
        compresses("after a refused second queue")
        comp.set_device_limit(0)
        q.close()
        q = None
        comp.trim()
        assert comp.device_bytes() == 0
    finally:
        if q is not None:
            q.close()
        comp.close()
