"""The sized compress queue (sz4_cq_create_sized / sz4_cq_enqueue_sized, Compressor.compress_queue_sized) on
the GPU: capacities fixed at create, the sizes of every enqueue read from a device table by the kernels.
Expected bytes come only from the oracle on the host model's split of the first n bytes
(oz_block(planes.split(item[:n], E), chain)); every comparison is byte-for-byte, addresses, sizes, statuses
and total included, inside a sentinel buffer.  The same queue is enqueued again and again with other sizes:
what a larger earlier run left in a slot (matches, marker bits, tokens, plan entries) must not show.
Data is text and increasing counters (no long same-byte runs: the oracle is quadratic there at levels 7 / 16).
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
OK, ARG, CAPACITY = _native.SZ4_ITEM_OK, _native.SZ4_ITEM_ARG, _native.SZ4_ITEM_CAPACITY
LDS_MAX = 65541
GARBAGE = 0x5A5A5A5A5A5A  # a source entry that must not be looked at


@pytest.fixture(scope="module")
def compressor(compressor):
    """The session's fixture decides whether there is a GPU; the tests here run on a context of their own."""
    import smallz4_amd
    c = smallz4_amd.Compressor(device=0)
    yield c
    c.close()


def numeric_bytes(n, seed):
    """Increasing int32 counters, then increasing int64 ones (tests/test_batch_typed.py)."""
    rng = np.random.default_rng(seed)
    a = (np.cumsum(rng.integers(0, 70000, n // 8 + 8)) & 0x7FFFFFFF).astype(np.int32).tobytes()
    b = np.cumsum(rng.integers(0, 2 ** 44, n // 16 + 8, dtype=np.int64)).astype(np.int64).tobytes()
    return (a + b)[:n]


@functools.lru_cache(maxsize=None)
def mixed_data(n, seed):
    """Text, then counters."""
    return synth.enwik8_like(n // 2, seed=seed) + numeric_bytes(n - n // 2, seed=seed + 1)


@functools.lru_cache(maxsize=None)
def block_of(data, E, chain):
    return pyoracle.oz_block(planes.split(data, E), chain) if data else b""


def oracle_blocks(items, elems, chain):
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda p: block_of(p[0], p[1], chain), zip(items, elems)))


def device_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


class Tables:
    """The device tables of one queue and its output: `bound` bytes, `lead` bytes into a larger tensor of 0xA5
    (tests/test_compress_queue.py's, with the size table of a sized queue)."""

    def __init__(self, q, lead=3, tail=256):
        import torch
        dev = "cuda:0"
        self.q, self.lead = q, lead
        self.whole = torch.full((lead + q.bound + tail,), SENTINEL, dtype=torch.uint8, device=dev)
        self.out = self.whole[lead:lead + q.bound]
        self.src = torch.zeros(q.count, dtype=torch.int64, device=dev)
        self.nsz = torch.zeros(q.count, dtype=torch.int32, device=dev)
        self.ptrs = torch.full((q.count,), -7, dtype=torch.int64, device=dev)
        self.sizes = torch.full((q.count,), -7, dtype=torch.int32, device=dev)
        self.status = torch.full((q.count,), -7, dtype=torch.int32, device=dev)
        self.total = torch.full((1,), -7, dtype=torch.int64, device=dev)

    def set(self, ptrs, sizes):
        """Rewrites both tables on the device (copies into the tensors an enqueue, or a captured one, names)."""
        import torch
        self.src.copy_(torch.tensor(list(ptrs), dtype=torch.int64))
        self.nsz.copy_(torch.tensor(list(sizes), dtype=torch.int32))

    def reset(self):
        self.whole.fill_(SENTINEL)
        self.ptrs.fill_(-7), self.sizes.fill_(-7), self.status.fill_(-7), self.total.fill_(-7)

    def enqueue(self):
        if hasattr(self.q, "capacities"):
            self.q.enqueue(self.src, self.nsz, self.out, self.ptrs, self.sizes, self.status, self.total)
        else:
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
        assert self.status.cpu().tolist() == (statuses or [OK] * len(want)), f"{what}: statuses"
        assert self.sizes.cpu().tolist() == [len(w) for w in want], f"{what}: block sizes"
        assert self.total.cpu().tolist() == [at], f"{what}: total"
        assert self.ptrs.cpu().tolist() == ptrs, f"{what}: block addresses"
        at = 0
        for i, w in enumerate(want):
            g = host[lead + at:lead + at + len(w)]
            if g != w:
                k = next(j for j in range(len(w)) if g[j] != w[j])
                pytest.fail(f"{what}: item {i} ({len(w)} block bytes) differs at offset {k}: {g[k:k + 8].hex()} for {w[k:k + 8].hex()}")
            at += len(w)
        assert host[:lead] == bytes([SENTINEL]) * lead, f"{what}: bytes before the output were written"
        assert host[lead + at:lead + bound] == bytes([SENTINEL]) * (bound - at), f"{what}: bytes after the last block were written"
        assert host[lead + bound:] == bytes([SENTINEL]) * (len(host) - lead - bound), f"{what}: bytes at or beyond the bound were written"


def run(t, data, base, offs, sizes, elems, chain, what):
    """One enqueue of sizes[i] bytes at data[offs[i]:] per slot, compared in full with the oracle."""
    t.reset()
    t.set([base.data_ptr() + o if n else GARBAGE for o, n in zip(offs, sizes)], sizes)
    t.enqueue()
    t.check(oracle_blocks([data[o:o + n] for o, n in zip(offs, sizes)], elems, chain), what=what)


# ---- 1. small slots, sizes sweeping the boundaries ----------------------------------------------
SMALL_CAP = 4200
SMALL_SLOTS = 24


def small_sizes(E):
    """24 sizes, large | small | empty | large in sixes: rotated by six per enqueue, a slot that starts in the
    first six goes large -> small -> empty -> large, and every other transition happens in some slot.  The 12-byte
    no-search edge, the 4096 walk sub-segment edge, the 4096-position parse segment edge (n - 5 = 4096 / 4097)
    and the full slot are all there."""
    s = [4200, 4102, 4101, 4097, 4096, 4095, 17, 13, 12, 11, E + 1, E, 0, 0, E - 1, 1, 0, 0, 4095, 4096, 4097, 4101, 4102, 4200]
    assert len(s) == SMALL_SLOTS and set(s) == {0, 1, E - 1, E, E + 1, 11, 12, 13, 17, 4095, 4096, 4097, 4101, 4102, 4200}
    return s


@pytest.mark.parametrize("chain", CHAINS)
def test_small_slots_over_four_enqueues(compressor, chain):
    elems = [WIDTHS[i % 4] for i in range(SMALL_SLOTS)]
    stride = SMALL_CAP + 40
    offs = [i * stride + (i - i * stride) % 16 for i in range(SMALL_SLOTS)]  # slot i at source alignment i mod 16
    data = mixed_data(SMALL_SLOTS * stride + 64, 171)
    base = device_bytes(data)
    assert {(base.data_ptr() + o) % 16 for o in offs} == set(range(16))
    q = compressor.compress_queue_sized([SMALL_CAP] * SMALL_SLOTS, elems, chain)
    try:
        assert q.count == SMALL_SLOTS and q.capacities == [SMALL_CAP] * SMALL_SLOTS
        assert q.bound == compressor.batch_bound([SMALL_CAP] * SMALL_SLOTS) == SMALL_SLOTS * (SMALL_CAP + 4)
        t = Tables(q)
        for r in range(4):
            sizes = [small_sizes(elems[i])[(i + 6 * r) % SMALL_SLOTS] for i in range(SMALL_SLOTS)]
            run(t, data, base, offs, sizes, elems, chain, f"chain {chain}, enqueue {r}")
    finally:
        q.close()


# ---- 2. the 64 KiB edge in one slot ---------------------------------------------------------------
@pytest.mark.parametrize("chain", [7, 65535])
def test_the_64k_edge_in_one_slot(compressor, chain):
    """Capacity 70000: the finders that read their window from HBM, two segments and 16 parse entries reserved;
    65536 bytes parse as 16 segments of 4096, 65537 as 8 of 8192; 65547 bytes have one segment, 65548 two."""
    sizes = [12, 65535, 65536, 65537, 65541, 65542, 65547, 65548, 70000]
    data = bytes(3) + mixed_data(70016, 173)  # the slot's source at alignment 3
    base = device_bytes(data)
    q = compressor.compress_queue_sized([70000], None, chain)
    try:
        t = Tables(q)
        for n in sizes + sizes[::-1]:
            run(t, data, base, [3], [n], [1], chain, f"chain {chain}, {n} bytes")
    finally:
        q.close()


# ---- 3. capacities that all fit the LDS finders ------------------------------------------------------
def test_capacities_that_fit_the_lds_finders(compressor):
    caps = [LDS_MAX, 65536]
    data = mixed_data(2 * 65600, 175)
    base = device_bytes(data)
    q = compressor.compress_queue_sized(caps, [1, 2], 65535)
    try:
        t = Tables(q)
        for sizes in ([LDS_MAX, 65536], [LDS_MAX - 1, 65535], [LDS_MAX, 65535], [LDS_MAX - 1, 65536]):
            run(t, data, base, [1, 65600], sizes, [1, 2], 65535, f"sizes {sizes}")
    finally:
        q.close()


# ---- 4. identity with the fixed queue ---------------------------------------------------------------
def sizes_for(E):
    return [0, 1, E - 1, E, E + 1, 15, 16, 17, 16 * E - 1, 16 * E, 16 * E + 1, 255, 256, 257, 1000, 4095, 4096, 4097,
            65535, 65536, LDS_MAX]


SETS = {
    "small": [(n, E) for E in WIDTHS for n in sizes_for(E)] + [(5000, 4), (5000, 2)],
    "mixed": [(1000, 1), (LDS_MAX, 1), (LDS_MAX + 1, 1), (70001, 1)],
}


@pytest.mark.parametrize("name,chain", [("small", 7), ("mixed", 65535)])
def test_identity_with_the_fixed_queue(compressor, name, chain):
    """Sizes equal to the capacities: bytes, addresses, sizes and total are compress_queue(caps)'s."""
    slices, at = [], 0
    for k, (n, E) in enumerate(SETS[name]):
        at += (k - at) % 16
        slices.append((at, n, E))
        at += n
    data = mixed_data(at + 64, 177)
    base = device_bytes(data)
    caps, elems = [n for _, n, _ in slices], [E for _, _, E in slices]
    results = []
    for make in (compressor.compress_queue, compressor.compress_queue_sized):
        q = make(caps, elems, chain)
        try:
            t = Tables(q)
            t.set([base.data_ptr() + a for a, _, _ in slices], caps)
            t.enqueue()
            import torch
            torch.cuda.synchronize()
            assert t.status.cpu().tolist() == [OK] * len(caps)
            total = int(t.total[0])
            results.append((q.bound, total, t.sizes.cpu().tolist(), [p - t.out.data_ptr() for p in t.ptrs.cpu().tolist()],
                            t.whole.cpu().numpy().tobytes()))
        finally:
            q.close()
    fixed, sized = results
    assert sized[:4] == fixed[:4]
    assert sized[4] == fixed[4]  # the whole buffer: the blocks, and the sentinel everywhere else
    assert fixed[1] == sum(fixed[2]) > 0


# ---- 5. statuses -------------------------------------------------------------------------------------
@pytest.mark.parametrize("elems", [None, [1, 4, 2, 8, 2]])
def test_statuses(compressor, elems):
    """Over capacity: SZ4_ITEM_CAPACITY and nothing written (its pointer is a live buffer: the test does not
    depend on a read being skipped).  A null source: zeros and SZ4_ITEM_ARG.  Size 0 with any pointer: empty."""
    caps = [3000, 1000, 2000, 1500, 800]
    data = mixed_data(9000, 179)
    base = device_bytes(data)
    e = elems or [1] * 5
    q = compressor.compress_queue_sized(caps, elems, 65535)
    try:
        t = Tables(q)
        p = base.data_ptr()
        t.set([p + 1, p + 3001, GARBAGE, 0, p + 8000], [3000, 1001, 0, 1500, 800])
        t.enqueue()
        want = [block_of(data[1:3001], e[0], 65535), b"", b"", block_of(bytes(1500), e[3], 65535),
                block_of(data[8000:8800], e[4], 65535)]
        t.check(want, statuses=[OK, CAPACITY, OK, ARG, OK], what=f"widths {elems}")
        # the same slots, all in order again: nothing of the refused enqueue is left
        t.reset()
        t.set([p + 1, p + 3001, p + 4001, p + 6001, p + 8000], [2999, 1000, 2000, 1, 0])
        t.enqueue()
        want = [block_of(data[1:3000], e[0], 65535), block_of(data[3001:4001], e[1], 65535),
                block_of(data[4001:6001], e[2], 65535), block_of(data[6001:6002], e[3], 65535), b""]
        t.check(want, what=f"widths {elems}, second enqueue")
    finally:
        q.close()


# ---- 6. bounds of the output ---------------------------------------------------------------------------
@pytest.mark.parametrize("lead", [0, 1, 16])
def test_nothing_is_written_at_or_beyond_the_bound(compressor, lead):
    """out is exactly `bound` long inside a larger buffer of 0xA5, at three alignments; the random item at full
    capacity is stored, so its block fills its share of the bound to the last byte."""
    data = synth.random_bytes(70001, seed=181)
    base = device_bytes(data)
    q = compressor.compress_queue_sized([70001, 0, 13], [1, 2, 4], 65535)
    try:
        t = Tables(q, lead=lead)
        assert t.out.numel() == q.bound == 70001 + 13 + 12
        t.set([base.data_ptr(), GARBAGE, base.data_ptr() + 100], [70001, 0, 13])
        t.enqueue()
        want = [block_of(data, 1, 65535), b"", block_of(data[100:113], 4, 65535)]
        assert sum(len(w) for w in want) == q.bound - 4  # stored blocks: only the empty slot's word is unused
        t.check(want, what=f"output {lead} bytes into its buffer")
    finally:
        q.close()


# ---- 7. graph capture ------------------------------------------------------------------------------------
def test_captured_enqueue_replays_on_rewritten_tables(compressor):
    """One enqueue of 64 slots captured and replayed four times; the pointer table AND the size table are
    rewritten on the device between the replays, and the result tables are read back between them.  Replay 2
    has empty and over-capacity items.  A synchronisation or an allocation inside the enqueue would fail the
    capture with a HIP error."""
    import torch
    count = 64
    caps = [4096 + (k * 977) % 61441 for k in range(count)]
    caps[0], caps[-1] = 4096, 65536
    elems = [WIDTHS[k % 4] for k in range(count)]
    data = mixed_data(2 << 20, 183)
    base = device_bytes(data)
    q = compressor.compress_queue_sized(caps, elems, 65535)
    try:
        t = Tables(q)
        t.set([base.data_ptr()] * count, caps)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            t.enqueue()
        rng = np.random.default_rng(184)
        for rep in range(4):
            offs = [((rep * 64 + k) * 48611 + 7 * rep + k) % (len(data) - 65536) for k in range(count)]
            if rep == 0:
                sizes = list(caps)
            else:
                sizes = [int(rng.integers(1, c // (1 if k % 3 else 8) + 1)) for k, c in enumerate(caps)]
            statuses = [OK] * count
            if rep == 2:
                for k in (0, 5, 17, 63):
                    sizes[k] = 0
                sizes[9] = caps[9] + 1
                statuses[9] = CAPACITY
            t.reset()
            t.set([base.data_ptr() + o for o in offs], sizes)
            g.replay()
            want = oracle_blocks([data[o:o + n] if s == OK else b"" for o, n, s in zip(offs, sizes, statuses)], elems, 65535)
            t.check(want, statuses=statuses, what=f"replay {rep}")
        del g
    finally:
        q.close()


# ---- 8. round trip in one graph ------------------------------------------------------------------------------
def test_round_trip_in_one_graph(compressor):
    """cq.enqueue (sized) -> dq.enqueue wired through block_ptrs / block_sizes in one captured graph: the chunk
    sizes of a bf16 tensor change between two replays, and every chunk decodes to its first n bytes."""
    import torch
    rng = np.random.default_rng(185)
    t = torch.from_numpy(rng.normal(0, 0.02, 100_003).astype(np.float32)).to(torch.bfloat16).cuda(0)
    chunk = 65536
    nbytes = t.numel() * 2
    caps = [min(chunk, nbytes - o) for o in range(0, nbytes, chunk)]
    count = len(caps)
    assert count == 4 and caps[-1] < chunk
    cq = compressor.compress_queue_sized(caps, [2] * count, 65535)
    dq = compressor.decode_queue(count, cq.bound)
    try:
        c = Tables(cq)
        c.src, c.nsz = cq.tensor_tables(t)
        assert c.src.cpu().tolist() == [t.data_ptr() + k * chunk for k in range(count)]
        assert c.nsz.dtype == torch.int32 and c.nsz.cpu().tolist() == caps
        back = torch.zeros_like(t)
        worst = [0]
        for n in caps:
            worst.append(worst[-1] + n + 4)
        d = dq.tensor_tables(CompressedTensor(c.out, worst, t.dtype, tuple(t.shape), chunk), back)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            c.enqueue()
            dq.enqueue(c.ptrs, c.sizes, d.dst_ptrs, d.dst_caps, d.out_sizes, d.status, elems=d.elems, count=count)
        raw = t.view(torch.uint8).cpu().numpy().tobytes()
        for rep, sizes in enumerate((caps, [40001, 65536, 12346, 2])):
            c.reset()
            c.nsz.copy_(torch.tensor(sizes, dtype=torch.int32))
            back.zero_()
            g.replay()
            torch.cuda.synchronize()
            assert c.status.cpu().tolist() == [OK] * count and d.status.cpu().tolist() == [OK] * count, f"replay {rep}"
            assert d.out_sizes.cpu().tolist() == sizes
            got = back.view(torch.uint8).cpu().numpy().tobytes()
            for k, n in enumerate(sizes):
                o = k * chunk
                assert got[o:o + n] == raw[o:o + n], f"replay {rep}, chunk {k}"
                assert got[o + n:o + caps[k]] == bytes(caps[k] - n), f"replay {rep}, chunk {k}: bytes past its size"
            c.check(oracle_blocks([raw[k * chunk:k * chunk + n] for k, n in enumerate(sizes)], [2] * count, 65535),
                    what=f"replay {rep}")
        del g
    finally:
        dq.close()
        cq.close()


# ---- 9. errors ---------------------------------------------------------------------------------------------------
def test_create_refuses(compressor):
    bad = [([], None, 65535), ([16] * 32769, None, 65535), ([100, (4 << 20) + 1], None, 65535), ([100, 100], [1, 3], 65535),
           ([100], None, 3), ([4 << 20] * 113, None, 65535)]
    for caps, elems, chain in bad:
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            compressor.compress_queue_sized(caps, elems, chain)
    for chain in (1, 6, 65536):
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            compressor.compress_queue_sized([100], None, chain)
    compressor.compress_queue_sized([100, 4 << 20], [8, 1], 7).close()  # the limits themselves are accepted
    compressor.compress_queue_sized([0] * 32768, None, 0).close()
    compressor.compress_queue_sized([16] * 32768, None, 7).close()


def test_wrong_enqueue_and_short_output_are_refused_before_any_work(compressor):
    import torch
    data = mixed_data(5000, 187)
    base = device_bytes(data)
    lib = _native.lib()
    import ctypes

    def untouched(t):
        torch.cuda.synchronize()
        assert bool((t.whole == SENTINEL).all())
        assert t.ptrs.cpu().tolist() == [-7, -7] and t.sizes.cpu().tolist() == [-7, -7]
        assert t.status.cpu().tolist() == [-7, -7] and t.total.cpu().tolist() == [-7]

    def raw(t, fn, with_sizes):
        p = lambda x: ctypes.c_void_p(x.data_ptr())
        args = [t.q._h, p(t.src)] + ([p(t.nsz)] if with_sizes else []) + \
            [p(t.out), t.out.numel(), p(t.ptrs), p(t.sizes), p(t.status), p(t.total), None]
        return getattr(lib, fn)(*args)

    sized = compressor.compress_queue_sized([3000, 2000], None, 65535)
    fixed = compressor.compress_queue([3000, 2000], None, 65535)
    try:
        for q in (sized, fixed):
            t = Tables(q)
            t.set([base.data_ptr(), base.data_ptr() + 3000], [3000, 2000])
            # the other kind's enqueue
            assert raw(t, "sz4_cq_enqueue" if q is sized else "sz4_cq_enqueue_sized", q is fixed) == _native.SZ4_E_ARG
            untouched(t)
        t = Tables(sized)
        t.set([base.data_ptr(), base.data_ptr() + 3000], [3000, 2000])
        # a null size table
        assert lib.sz4_cq_enqueue_sized(sized._h, ctypes.c_void_p(t.src.data_ptr()), None, ctypes.c_void_p(t.out.data_ptr()),
                                        t.out.numel(), ctypes.c_void_p(t.ptrs.data_ptr()), ctypes.c_void_p(t.sizes.data_ptr()),
                                        ctypes.c_void_p(t.status.data_ptr()), None, None) == _native.SZ4_E_ARG
        untouched(t)
        t.out = t.whole[t.lead:t.lead + sized.bound - 1]
        with pytest.raises(_native.NativeError, match=r"\(-3\)"):
            t.enqueue()
        untouched(t)
    finally:
        sized.close()
        fixed.close()


# ---- 10. lifetime ------------------------------------------------------------------------------------------------
def test_limits_and_lifetime(compressor):
    """A context of its own, so that its device bytes are the queue's and this test's alone."""
    import smallz4_amd
    comp = smallz4_amd.Compressor(device=0)
    q = None
    try:
        assert comp.device_bytes() == 0
        n, count = 65536, 8
        data = mixed_data(n * count, 189)
        base = device_bytes(data)
        q = comp.compress_queue_sized([n] * count, None, 65535)
        held = comp.device_bytes()
        assert held >= 36 * n * count
        t = Tables(q)
        offs = [k * n for k in range(count)]

        def compresses(sizes, what):
            run(t, data, base, offs, sizes, [1] * count, 65535, what)

        compresses([n] * count, "after create")
        comp.compress_batch([data[:5000], data[5000:70000]], 3)
        assert comp.device_bytes() > held
        comp.trim()
        assert comp.device_bytes() == held  # trim leaves the queue's scratch, and only that
        compresses([n - 7 * k for k in range(count)], "after trim")
        comp.set_device_limit(comp.device_bytes())
        with pytest.raises(_native.NativeError, match=r"\(-4\)"):
            comp.compress_queue_sized([n] * count, None, 65535)
        assert comp.device_bytes() == held
        compresses([n] * count, "after a refused second queue")
        comp.set_device_limit(0)
        q.close()
        q = None
        comp.trim()
        assert comp.device_bytes() == 0
    finally:
        if q is not None:
            q.close()
        comp.close()
