"""The decode queue (sz4_dq_*, Compressor.decode_queue) on the GPU: device tables of pointers in, decoded
items, sizes and per-item statuses out, nothing on the host in between.  Every item lives in a tensor of its
own -- the source at a chosen alignment, the destination inside a larger tensor filled with 0xA5, so that
the bytes before it and after its capacity show any store that strays.  Expected bytes come from
lz4seq.expand() (tests/test_lz4seq_model.py pins it to the oracle and the reference), from the host model
planes.merge, and from the synchronous batch calls this queue must agree with.  Run with -m gpu on an MI355X."""
import functools
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

import lz4seq
from oracle import pyoracle
from smallz4_amd import _native, planes, synth

pytestmark = pytest.mark.gpu

FAMILIES = ["overlap", "lengths", "counts", "windows", "ring", "below", "split", "random"]
SENTINEL = 0xA5
PAD = 64
OK, CORRUPT, CAPACITY, ARG, QUEUE = (_native.SZ4_ITEM_OK, _native.SZ4_ITEM_CORRUPT, _native.SZ4_ITEM_CAPACITY,
                                     _native.SZ4_ITEM_ARG, _native.SZ4_ITEM_QUEUE)
QUEUE_ITEMS = 4096
QUEUE_BYTES = 32 << 20


@pytest.fixture(scope="module")
def compressor(compressor):
    """The session's fixture decides whether there is a GPU; the tests here run on a context of their own, so
    that what they grow in it (batch scratch, decoder lists) is gone when the module ends and no later test
    finds the shared context in another state than before."""
    import smallz4_amd
    c = smallz4_amd.Compressor(device=0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def queue(compressor):
    q = compressor.decode_queue(QUEUE_ITEMS, QUEUE_BYTES)
    yield q
    q.close()


def item_of(word, payload):
    return struct.pack("<I", word) + payload


def device_bytes(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


class Batch:
    """Items in tensors of their own and the device tables over them.  Item k's source starts `align[k]` bytes
    into its tensor (default k mod 8); its destination starts PAD + dst_off[k] bytes into a tensor of 0xA5
    (default: an odd offset) that ends PAD bytes after its capacity.  null_src / null_dst: item indices whose
    pointer is null."""

    def __init__(self, items, caps, elems=None, align=None, dst_off=None, null_src=(), null_dst=()):
        import torch
        self.n = len(items)
        self.caps = list(caps)
        self.lead = [PAD + (dst_off[k] if dst_off else 1 + 2 * (k % 5)) for k in range(self.n)]
        self.src, self.dst = [], []
        sp, dp = [], []
        for k, it in enumerate(items):
            a = align[k] if align else k % 8
            s = device_bytes(bytes(a) + bytes(it) + bytes(8))
            d = torch.full((self.lead[k] + self.caps[k] + PAD,), SENTINEL, dtype=torch.uint8, device="cuda:0")
            assert s.data_ptr() % 16 == 0 and d.data_ptr() % 16 == 0
            self.src.append(s)
            self.dst.append(d)
            sp.append(0 if k in null_src else s.data_ptr() + a)
            dp.append(0 if k in null_dst else d.data_ptr() + self.lead[k])
        dev = "cuda:0"
        self.src_ptrs = torch.tensor(sp, dtype=torch.int64).to(dev)
        self.src_sizes = torch.tensor([len(it) for it in items], dtype=torch.int32).to(dev)
        self.dst_ptrs = torch.tensor(dp, dtype=torch.int64).to(dev)
        self.dst_caps = torch.tensor(self.caps, dtype=torch.int32).to(dev)
        self.elems = None if elems is None else torch.tensor(list(elems), dtype=torch.uint8).to(dev)
        self.out_sizes = torch.full((self.n,), -7, dtype=torch.int32, device=dev)
        self.status = torch.full((self.n,), -7, dtype=torch.int32, device=dev)

    def run(self, q):
        import torch
        q.enqueue(self.src_ptrs, self.src_sizes, self.dst_ptrs, self.dst_caps, self.out_sizes, self.status, elems=self.elems)
        torch.cuda.synchronize()
        self.sizes = self.out_sizes.cpu().tolist()
        self.st = self.status.cpu().tolist()
        self.host = [d.cpu().numpy().tobytes() for d in self.dst]
        return self

    def check(self, k, want, what=""):
        """Item k decoded to `want`, and nothing else of its tensor was written."""
        assert self.st[k] == OK, f"{what}: item {k} has status {self.st[k]}"
        assert self.sizes[k] == len(want), f"{what}: item {k} reports {self.sizes[k]} bytes for {len(want)}"
        h, lead = self.host[k], self.lead[k]
        got = h[lead:lead + len(want)]
        if got != want:
            at = next(i for i in range(len(want)) if got[i] != want[i])
            pytest.fail(f"{what}: item {k} differs at output offset {at} of {len(want)}: "
                        f"{got[at:at + 8].hex()} for {want[at:at + 8].hex()}")
        assert h[:lead] == bytes([SENTINEL]) * lead, f"{what}: item {k}: bytes before the destination were written"
        rest = len(h) - lead - len(want)
        assert h[lead + len(want):] == bytes([SENTINEL]) * rest, f"{what}: item {k}: bytes after the output were written"

    def untouched(self, k, what=""):
        assert self.host[k] == bytes([SENTINEL]) * len(self.host[k]), f"{what}: item {k}'s destination was written"


# ---- 1. conformance --------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
def test_conformance(queue, family):
    """Every block of every well-formed case an item of its own, from a zero history: source alignments 0-7,
    odd destination addresses, capacity exact or 7 bytes more."""
    cases = [c for c in lz4seq.well_formed(family) if not c.dictionary]
    assert cases
    items, want, names = [], [], []
    for case in cases:
        for k, (word, payload) in enumerate(case.items()):
            items.append(item_of(word, payload))
            want.append(lz4seq.expand([case.blocks[k]], independent=True))
            names.append(f"{case} block {k}")
    assert sum(len(i) for i in items) <= QUEUE_BYTES and len(items) <= QUEUE_ITEMS
    caps = [len(w) + (7 if k % 2 else 0) for k, w in enumerate(want)]
    b = Batch(items, caps).run(queue)
    assert {p % 8 for p in b.src_ptrs.cpu().tolist()} == set(range(min(8, len(items))))
    assert all(p % 2 == 1 for p in b.dst_ptrs.cpu().tolist())
    for k, w in enumerate(want):
        b.check(k, w, names[k])


# ---- 2. malformed ----------------------------------------------------------------------------
def good_items():
    a = synth.enwik8_like(3000, seed=91)
    return [pyoracle.oz_block(a[:1700], 65535), pyoracle.oz_block(a[1700:], 3)], [a[:1700], a[1700:]]


def test_malformed_items_fail_alone(queue, compressor):
    (g0, g1), (w0, w1) = good_items()
    bad = [item_of(*case.items()[0]) for case in lz4seq.malformed()]
    names = [repr(c) for c in lz4seq.malformed()]
    assert all(len(c.items()) == 1 for c in lz4seq.malformed())
    # an extent shorter than the size word, and size words that disagree with the extent
    for n in (1, 2, 3):
        bad.append(g0[:n])
        names.append(f"extent of {n} bytes")
    bad += [g0 + b"\0", g0[:-1], struct.pack("<I", len(g0) - 4 + 1) + g0[4:], struct.pack("<I", 0) + g0[4:]]
    names += ["extent one byte longer", "extent one byte shorter", "size word one more", "zero size word over a payload"]
    items, caps = [], []
    for x in bad:
        items += [g0, x, g1]
        caps += [len(w0), 70000, len(w1)]
    b = Batch(items, caps).run(queue)
    for j, name in enumerate(names):
        b.check(3 * j, w0, f"before {name}")
        b.check(3 * j + 2, w1, f"after {name}")
        assert b.st[3 * j + 1] == CORRUPT, f"{name}: status {b.st[3 * j + 1]}"
        assert b.sizes[3 * j + 1] == 0
        b.untouched(3 * j + 1, name)
        with pytest.raises(_native.NativeError, match=r"\(-6\)"):  # SZ4_E_CORRUPT from the synchronous call
            compressor.unlz4_batch([g0, bad[j], g1])


# ---- 3. capacity and null pointers -----------------------------------------------------------
def test_capacity_and_null_pointers(queue):
    (g0, g1), (w0, w1) = good_items()
    n0 = len(w0)
    empty_block = struct.pack("<I", 0)  # a zero word alone: decodes to nothing
    items = [g0, g0, g0, g0, g1, g0, b"", empty_block, b""]
    caps = [n0 - 1, n0, n0 + 7, 0, len(w1), n0, 0, 0, 5]
    b = Batch(items, caps, null_dst=(3, 7, 8), null_src=(5, 8)).run(queue)
    assert (b.st[0], b.sizes[0]) == (CAPACITY, n0)
    b.untouched(0, "capacity one byte short")
    b.check(1, w0, "capacity exact")
    b.check(2, w0, "capacity + 7")
    assert (b.st[3], b.sizes[3]) == (CAPACITY, n0)  # a null destination of capacity 0
    b.check(4, w1, "after the failed items")
    assert (b.st[5], b.sizes[5]) == (ARG, 0)  # a null source of non-zero size
    b.untouched(5, "null source")
    assert (b.st[6], b.sizes[6]) == (OK, 0)
    b.untouched(6, "empty item")
    assert (b.st[7], b.sizes[7]) == (OK, 0)  # nothing to store: the null destination is never needed
    assert (b.st[8], b.sizes[8]) == (OK, 0)  # an empty item: neither pointer is looked at


# ---- 4. typed items --------------------------------------------------------------------------
def sizes_for(E):
    """tests/test_batch_typed.py's ragged sizes: whole elements, tails, n < E, empty."""
    return [0, 1, E - 1, E, E + 1, 15, 16, 17, 16 * E - 1, 16 * E, 16 * E + 1, 255, 256, 257, 1000, 4095, 4096, 4097,
            65535, 65536, 65537, 70001, 200003]


def numeric_bytes(n, seed):
    rng = np.random.default_rng(seed)
    a = (np.cumsum(rng.integers(0, 70000, n // 8 + 8)) & 0x7FFFFFFF).astype(np.int32).tobytes()
    b = np.cumsum(rng.integers(0, 2 ** 44, n // 16 + 8, dtype=np.int64)).astype(np.int64).tobytes()
    return (a + b)[:n]


@functools.lru_cache(maxsize=None)
def typed_case(chain=3):
    """(items, widths, oracle blocks of their splits)."""
    data = synth.enwik8_like(300_000, seed=92) + numeric_bytes(300_000, seed=93)
    items, elems, at = [], [], 0
    for E in planes.WIDTHS:
        for n in sizes_for(E):
            at = (at * 7 + 13) % (len(data) - n)
            items.append(data[at:at + n])
            elems.append(E)
    with ThreadPoolExecutor(max_workers=8) as ex:
        blocks = list(ex.map(lambda p: pyoracle.oz_block(planes.split(p[0], p[1]), chain) if p[0] else b"", zip(items, elems)))
    return items, elems, blocks


def test_typed_ragged(queue):
    items, elems, blocks = typed_case()
    # destinations at multiples of the width and at odd addresses, in turn
    dst_off = [(E * (k % 3 + 1) if k % 2 else 1 + 2 * (k % 5)) for k, E in enumerate(elems)]
    b = Batch(blocks, [len(x) + (k % 3) for k, x in enumerate(items)], elems=elems, dst_off=dst_off).run(queue)
    for k, x in enumerate(items):
        b.check(k, x, f"{len(x)} bytes of width {elems[k]}")
    # the same blocks at width 1 are their splits
    b = Batch(blocks, [len(x) for x in items], elems=[1] * len(items)).run(queue)
    for k, x in enumerate(items):
        b.check(k, planes.split(x, elems[k]), f"the split of {len(x)} bytes of width {elems[k]}")


@pytest.mark.parametrize("family", ["ring", "below"])
def test_typed_constructed(queue, family):
    """Blocks built to read drained output beyond the ring, and below their start, taken as splits: the
    mapped reads and the zero history."""
    items, want, elems, names = [], [], [], []
    for case in lz4seq.well_formed(family):
        if case.dictionary:
            continue
        for k, (word, payload) in enumerate(case.items()):
            flat = lz4seq.expand([case.blocks[k]], independent=True)
            for E in (2, 4, 8):
                items.append(item_of(word, payload))
                want.append(planes.merge(flat, E))
                elems.append(E)
                names.append(f"{case} block {k} at width {E}")
    b = Batch(items, [len(w) for w in want], elems=elems).run(queue)
    for k, w in enumerate(want):
        b.check(k, w, names[k])


def test_bad_width_fails_alone(queue):
    (g0, g1), (w0, w1) = good_items()
    b = Batch([g0, g1, g0, g1], [len(w0), len(w1), len(w0), len(w1)], elems=[1, 0, 3, 1]).run(queue)
    b.check(0, w0)
    b.check(3, w1)
    for k in (1, 2):
        assert (b.st[k], b.sizes[k]) == (ARG, 0)
        b.untouched(k, "bad width")


# ---- 5. against the synchronous path ---------------------------------------------------------
@functools.lru_cache(maxsize=None)
def text_items():
    data = synth.enwik8_like(6 << 20, seed=94)
    rng = np.random.default_rng(95)
    items = []
    for _ in range(200):
        n = int(rng.integers(1 << 10, (256 << 10) + 1))
        at = int(rng.integers(0, len(data) - n))
        items.append(data[at:at + n])
    items.append(data[5:5 + (4 << 20)])
    return items


def test_against_unlz4_batch(queue, compressor):
    items = text_items()
    blocks = compressor.compress_batch(items, 3)
    assert sum(len(x) for x in blocks) <= QUEUE_BYTES
    want = compressor.unlz4_batch(blocks)
    assert want == items
    b = Batch(blocks, [len(x) for x in items]).run(queue)
    for k, w in enumerate(want):
        b.check(k, w, f"item {k}")


def test_against_unlz4_batch_typed(queue, compressor):
    items = text_items()[:60] + [numeric_bytes(n, 96 + n % 7) for n in (1000, 65536, 200001, 1 << 20)] + text_items()[-1:]
    elems = [planes.WIDTHS[k % 4] for k in range(len(items))]
    blocks = compressor.compress_batch_typed(items, elems, 3)
    want = compressor.unlz4_batch_typed(blocks, elems)
    assert want == items
    b = Batch(blocks, [len(x) for x in items], elems=elems).run(queue)
    for k, w in enumerate(want):
        b.check(k, w, f"item {k} of width {elems[k]}")


# ---- 6. graph capture ------------------------------------------------------------------------
def test_captured_enqueue_replays_on_rewritten_tables(queue, compressor):
    """One enqueue of 64 slots captured on torch's capture stream, replayed three times over rewritten tables.
    A synchronisation or an allocation inside the enqueue would fail the capture with a HIP error."""
    import torch
    slots = 64
    items, elems, blocks = typed_case()
    pool = [k for k, x in enumerate(items) if 0 < len(x) <= 70001]
    dev = "cuda:0"
    src = [device_bytes(blocks[k]) for k in pool]
    room = 70001 + 2 * PAD
    dest = torch.empty(slots * room, dtype=torch.uint8, device=dev)
    t_src = torch.zeros(slots, dtype=torch.int64, device=dev)
    t_dst = torch.zeros(slots, dtype=torch.int64, device=dev)
    t_ssz = torch.zeros(slots, dtype=torch.int32, device=dev)
    t_cap = torch.zeros(slots, dtype=torch.int32, device=dev)
    t_el = torch.ones(slots, dtype=torch.uint8, device=dev)
    t_out = torch.zeros(slots, dtype=torch.int32, device=dev)
    t_st = torch.zeros(slots, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        queue.enqueue(t_src, t_ssz, t_dst, t_cap, t_out, t_st, elems=t_el, count=slots)
    for rep, used in enumerate((64, 5, 37)):
        pick = [pool[(rep * 17 + 3 * j) % len(pool)] for j in range(used)]
        sp = [src[pool.index(k)].data_ptr() for k in pick] + [0] * (slots - used)
        ss = [len(blocks[k]) for k in pick] + [0] * (slots - used)
        dp = [dest.data_ptr() + j * room + PAD + 1 for j in range(slots)]
        cp = [len(items[k]) for k in pick] + [0] * (slots - used)
        el = [elems[k] for k in pick] + [1] * (slots - used)
        t_src.copy_(torch.tensor(sp, dtype=torch.int64))
        t_ssz.copy_(torch.tensor(ss, dtype=torch.int32))
        t_dst.copy_(torch.tensor(dp, dtype=torch.int64))
        t_cap.copy_(torch.tensor(cp, dtype=torch.int32))
        t_el.copy_(torch.tensor(el, dtype=torch.uint8))
        t_out.fill_(-7)
        t_st.fill_(-7)
        dest.fill_(SENTINEL)
        g.replay()
        torch.cuda.synchronize()
        host = dest.cpu().numpy().tobytes()
        assert t_st.cpu().tolist() == [OK] * slots, f"replay {rep}"
        assert t_out.cpu().tolist() == cp, f"replay {rep}"
        for j in range(slots):
            want = items[pick[j]] if j < used else b""
            h = host[j * room:(j + 1) * room]
            assert h[PAD + 1:PAD + 1 + len(want)] == want, f"replay {rep}, slot {j}"
            assert h[:PAD + 1] == bytes([SENTINEL]) * (PAD + 1), f"replay {rep}, slot {j}"
            assert h[PAD + 1 + len(want):] == bytes([SENTINEL]) * (room - PAD - 1 - len(want)), f"replay {rep}, slot {j}"
    del g


# ---- 7. limits and lifetime ------------------------------------------------------------------
def test_limits_and_lifetime(compressor):
    """A context of its own, so that its device bytes are the queue's and this test's alone."""
    import smallz4_amd
    comp = smallz4_amd.Compressor(device=0)
    q = None
    try:
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            comp.decode_queue(0, 1 << 20)
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            comp.decode_queue(65537, 1 << 20)
        assert comp.device_bytes() == 0
        (g0, g1), (w0, w1) = good_items()
        max_src = 3 * len(g0) + len(g1) + 10
        q = comp.decode_queue(16, max_src)
        held = comp.device_bytes()
        assert held >= 16 * 8 + (max_src // 3) * 16  # the list offsets and the sequence lists at least

        def decodes():
            b = Batch([g0, g1, b"", g0], [len(w0), len(w1), 0, len(w0)]).run(q)
            b.check(0, w0)
            b.check(1, w1)
            b.check(3, w0)

        decodes()
        # more items than the queue holds: refused before any device work
        many = Batch([g1] * 17, [len(w1)] * 17)
        with pytest.raises(_native.NativeError, match=r"\(-1\)"):
            many.run(q)
        assert many.status.cpu().tolist() == [-7] * 17
        # the source bytes pass max_src_bytes inside the fifth item: it and every later one are refused
        b = Batch([g0, g1, g0, g0, g1, b"", g1], [len(w0), len(w1), len(w0), len(w0), len(w1), 0, len(w1)]).run(q)
        for k, w in enumerate((w0, w1, w0, w0)):
            b.check(k, w, "before the bound")
        for k in (4, 5, 6):
            assert (b.st[k], b.sizes[k]) == (QUEUE, 0)
            b.untouched(k, "past the bound")
        # trim leaves the queue's scratch, and only that
        comp.compress_batch([w0, w1], 3)
        assert comp.device_bytes() > held
        comp.trim()
        assert comp.device_bytes() == held
        decodes()
        # a synchronous call that has to shed under a bound leaves it too
        blocks = comp.compress_batch([w0, w1], 3)
        shed = comp.released_buffers()
        comp.set_device_limit(comp.device_bytes())
        assert comp.unlz4_batch(blocks) == [w0, w1]
        assert comp.released_buffers() > shed
        assert comp.device_bytes() >= held
        decodes()
        # a second queue over the bound
        with pytest.raises(_native.NativeError, match=r"\(-4\)"):
            comp.decode_queue(16, 1 << 30)
        decodes()
        comp.set_device_limit(0)
        q.close()
        q = None
        comp.trim()
        assert comp.device_bytes() == 0
    finally:
        if q is not None:
            q.close()
        comp.close()


# ---- 8. tensors ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["bf16", "fp32", "int64"])
def test_tensor_tables(queue, compressor, name):
    import torch
    rng = np.random.default_rng(97)
    t = {"bf16": lambda: torch.from_numpy(rng.normal(0, 0.02, 100_003).astype(np.float32)).to(torch.bfloat16),
         "fp32": lambda: torch.from_numpy(rng.normal(0, 0.02, (257, 129)).astype(np.float32)),
         "int64": lambda: torch.from_numpy((1_700_000_000_000 + np.cumsum(rng.integers(1, 1000, 20_001))).astype(np.int64)),
         }[name]().cuda(0)
    ct = compressor.compress_tensor(t)
    nbytes = t.numel() * t.element_size()
    assert nbytes % ct.chunk_bytes and len(ct.offsets) - 1 == nbytes // ct.chunk_bytes + 1  # the last chunk is shorter
    out = torch.zeros_like(t)
    tables = queue.tensor_tables(ct, out)
    assert tables.count == len(ct.offsets) - 1
    for _ in range(2):  # the tables serve any number of enqueues
        out.zero_()
        queue.enqueue_tables(tables)
        torch.cuda.synchronize()
        assert tables.status.cpu().tolist() == [OK] * tables.count
        assert sum(tables.out_sizes.cpu().tolist()) == nbytes
        assert bool((out.view(torch.uint8) == t.view(torch.uint8)).all())
