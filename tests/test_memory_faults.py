"""The host driver's out-of-memory paths on the GPU: the piece-halving retries of the
blocks and batch entry points, the allocator branch of DevBuf::reserve, the free-memory cap of the piece sizing,
and a failed reservation at every growth of every kind of call.  Failures are injected by the accounting's test
hooks (SZ4_TEST_ALLOC_CAP, SZ4_TEST_FAIL_RESERVE, SZ4_TEST_FREE_BYTES, read when a context is created), which
only ever make a context allocate less.  Expected bytes come from the oracle alone; a call either gives them or
returns SZ4_E_NOMEM with a message.  Any other error status ends the module: nothing more is started on the GPU
after a device error.  Run with -m gpu on an MI355X."""
import functools
import os
import re

import numpy as np
import pytest

from oracle import pyoracle
from smallz4_amd import _native, planes, synth

pytestmark = pytest.mark.gpu

MiB = 1 << 20
OK, NOMEM = _native.SZ4_OK, _native.SZ4_E_NOMEM
BYTES, BITS = _native.SZ4_FILTER_BYTES, _native.SZ4_FILTER_BITS
HEADER = bytes([0x04, 0x22, 0x4D, 0x18, 0x40, 0x70, 0xDF])
HOOKS = ("SZ4_TEST_ALLOC_CAP", "SZ4_TEST_FAIL_RESERVE", "SZ4_TEST_FREE_BYTES", "SZ4_UNLZ4_SPLIT")

_halt = []  # the first status that was neither SZ4_OK nor SZ4_E_NOMEM


@pytest.fixture(autouse=True)
def _nothing_after_a_device_error():
    if _halt:
        pytest.skip("an earlier case ended with a device error, nothing more runs on the GPU: " + _halt[0])


def context(**env):
    """A context of its own, created with these hook variables set (and removed right after)."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import smallz4_amd
    assert set(env) <= set(HOOKS)
    for k, v in env.items():
        os.environ[k] = str(int(v))
    try:
        return smallz4_amd.Compressor(device=0)
    finally:
        for k in env:
            del os.environ[k]


def attempt(fn):
    """(status, value, message) of a call through the Python wrappers, which raise NativeError("... failed (rc): message")."""
    try:
        return OK, fn(), ""
    except _native.NativeError as e:
        m = re.search(r"failed \((-?\d+)\)(?:: (.*))?", str(e), re.S)
        rc = int(m.group(1)) if m else None
        if rc != NOMEM:
            _halt.append(str(e))
            pytest.fail(f"a status other than SZ4_OK / SZ4_E_NOMEM: {e}")
        return rc, None, m.group(2) or ""
    except RuntimeError as e:  # the runtime's own error (torch): the same end
        _halt.append(str(e))
        raise


def succeed(fn):
    rc, value, msg = attempt(fn)
    assert rc == OK, msg
    return value


def on_device(data):
    import torch
    return torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda(0)


# ---- the 64 MiB inputs: sixteen distinct 64 KiB blocks tiled with period 1 MiB --------------------------
@functools.lru_cache(maxsize=None)
def tile():
    data = synth.enwik8_like(MiB, seed=91)
    return data, tuple(pyoracle.oz_block(data[k << 16:(k + 1) << 16], 65535) for k in range(16))


def tiled_frame(mib):
    """What compress_blocks gives for the tile repeated `mib` times: block k is the oracle's block k mod 16."""
    return HEADER + b"".join(tile()[1]) * mib + b"\0\0\0\0"


def tiled_sizes(mib):
    return [len(b) for b in tile()[1]] * mib


@functools.lru_cache(maxsize=None)
def tiled_device(mib):
    return on_device(tile()[0]).repeat(mib)


@functools.lru_cache(maxsize=None)
def blocks_needs():
    """device_bytes() of two unhooked contexts after 64 MiB in 16 MiB and in 32 MiB pieces (sizings, no criteria);
    both frames are the oracle's."""
    need = []
    for piece in (16 * MiB, 32 * MiB):
        comp = context()
        try:
            comp.set_batch_chunk(piece)
            rc, frame, msg = attempt(lambda: comp.compress_blocks(tiled_device(64), 65536, 65535))
            assert rc == OK, msg
            assert frame == tiled_frame(64)
            assert comp.debug_memory()["retries"] == 0 and comp.debug_memory()["min_piece"] == piece
            need.append(comp.device_bytes())
        finally:
            comp.close()
    return tuple(need)


# ---- a. the blocks retry, two halvings -------------------------------------------------------------------
def test_blocks_retry_halves_twice_under_a_capacity():
    """64 MiB in one 64 MiB piece on a device that holds 1.25 x what 16 MiB pieces need: the piece is halved
    twice, and the retry at 16 MiB has to succeed as a fresh context does under the same capacity -- it does
    only if the buffers the larger attempts grew are released first.  Without that release (the driver before
    this test) the call failed at the floor, as ADVICE.md read it: measured need16 = 609 258 293, need32 =
    1 218 410 837, cap = 761 572 866 bytes; after 2 retries SZ4_E_NOMEM "device allocation: out of memory" with
    696 774 374 bytes of the larger attempts still held."""
    need16, need32 = blocks_needs()
    cap = need16 * 5 // 4
    print(f"need16 {need16} need32 {need32} cap {cap}")
    assert cap < need32
    data = tile()[0] * 64
    comp = context(SZ4_TEST_ALLOC_CAP=cap)
    try:
        comp.set_batch_chunk(64 * MiB)
        rc, frame, msg = attempt(lambda: comp.compress_blocks(tiled_device(64), 65536, 65535))
        mem = comp.debug_memory()
        print(f"first call: status {rc} {msg!r} {mem} device_bytes {comp.device_bytes()}")
        assert rc == OK, msg
        assert frame == tiled_frame(64)
        assert comp.last_block_sizes(1024) == tiled_sizes(64)
        assert mem["retries"] == 2 and mem["min_piece"] == 16 * MiB
        assert mem["injected"] >= 2
        assert comp.device_bytes() <= cap
        assert comp.last_error() == ""
        # the same context again, the hook still set: the same bytes, and no more retries than a context new to
        # this capacity needs (the piece sizing starts from 64 MiB again: 2)
        rc, again, msg = attempt(lambda: comp.compress_blocks(tiled_device(64), 65536, 65535))
        mem = comp.debug_memory()
        print(f"second call: status {rc} {msg!r} {mem}")
        assert rc == OK, msg
        assert again == frame
        assert mem["retries"] <= 2 and mem["min_piece"] == 16 * MiB
        assert comp.device_bytes() <= cap and comp.last_error() == ""
    finally:
        comp.close()
    plain = context()
    try:
        assert succeed(lambda: plain.unlz4(frame)) == data
    finally:
        plain.close()


# ---- b. the blocks retry at offset 0 -----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blocks_growths():
    """Growths of 40 MiB in two 20 MiB pieces, and of 20 MiB in one, on contexts new to it."""
    g = []
    for mib in (40, 20):
        comp = context()
        try:
            comp.set_batch_chunk(20 * MiB)
            assert succeed(lambda: comp.compress_blocks(tiled_device(mib), 65536, 65535)) == tiled_frame(mib)
            g.append(comp.debug_memory()["growths"])
        finally:
            comp.close()
    return tuple(g)


@pytest.mark.parametrize("where", ["first growth", "last growth"])
def test_blocks_retry_in_the_first_piece(where):
    """40 MiB in 20 MiB pieces, a growth of the first piece fails (its first, the block table; its last, the
    staging): the offset steps back through the unsigned wrap, and the call runs 16 + 16 + 8 MiB; every block
    and every reported size is the oracle's."""
    g40, _ = blocks_growths()
    comp = context(SZ4_TEST_FAIL_RESERVE=1 if where == "first growth" else g40)
    try:
        comp.set_batch_chunk(20 * MiB)
        rc, frame, msg = attempt(lambda: comp.compress_blocks(tiled_device(40), 65536, 65535))
        assert rc == OK, msg
        assert frame == tiled_frame(40)
        assert comp.last_block_sizes(1024) == tiled_sizes(40)
        mem = comp.debug_memory()
        assert mem["injected"] == 1 and mem["retries"] == 1 and mem["min_piece"] == 16 * MiB
        assert comp.last_error() == ""
    finally:
        comp.close()


def test_blocks_later_pieces_do_not_grow():
    """The pieces of a call are equal (the last one no larger), so every buffer has its size after the first:
    the second piece reserves without reaching the allocator, and a failed reservation cannot land there.  (A
    retry at a later offset needs an allocator that fails where nothing is asked of it; the hooks cannot, and do
    not, produce one.)"""
    g40, g20 = blocks_growths()
    assert g40 == g20


# ---- c. the ragged batch retry ---------------------------------------------------------------------------
def batch_call(comp, kind, base, count=64):
    """64 items of 1 MiB (the tile each): (raw bytes, offsets)."""
    import torch
    sizes = [MiB] * count
    ptrs = [base.data_ptr() + i * MiB for i in range(count)]
    cap = comp.batch_bound(sizes)
    out = torch.empty(cap, dtype=torch.uint8, device="cuda:0")
    if kind == "plain":
        off = comp.compress_batch_device(ptrs, sizes, out.data_ptr(), cap, 65535)
    elif kind in ("typed2", "typed4"):
        off = comp.compress_batch_typed_device(ptrs, sizes, [int(kind[-1])] * count, out.data_ptr(), cap, 65535)
    else:  # one item in its bit planes, the others in their byte planes, width 2; level 3 (see batch_expected)
        off = comp.compress_batch_filtered_device(ptrs, sizes, [2] * count, [BITS if i == 5 else BYTES for i in range(count)],
                                                  out.data_ptr(), cap, 3)
    return out[:off[-1]].cpu().numpy().tobytes(), off


@functools.lru_cache(maxsize=None)
def batch_expected(kind):
    """The 64 blocks.  The bit planes of text are long runs, on which the oracle's level 9 is quadratic: that call
    runs at level 3, whose retry and scratch are the same."""
    t = tile()[0]
    if kind == "plain":
        return (pyoracle.oz_block(t, 65535),) * 64
    if kind in ("typed2", "typed4"):
        return (pyoracle.oz_block(planes.split(t, int(kind[-1])), 65535),) * 64
    b = [pyoracle.oz_block(planes.split(t, 2), 3)] * 64
    b[5] = pyoracle.oz_block(planes.bit_split(t, 2), 3)
    return tuple(b)


@functools.lru_cache(maxsize=None)
def batch_needs():
    need = []
    for piece in (16 * MiB, 32 * MiB):
        comp = context()
        try:
            comp.set_batch_chunk(piece)
            rc, res, msg = attempt(lambda: batch_call(comp, "plain", tiled_device(64)))
            assert rc == OK, msg
            assert res[0] == b"".join(batch_expected("plain"))
            need.append(comp.device_bytes())
        finally:
            comp.close()
    return tuple(need)


@pytest.mark.parametrize("kind", ["plain", "typed2", "typed4", "bits"])
def test_batch_retry_under_a_capacity(kind):
    need16, need32 = batch_needs()
    cap = need16 * 5 // 4
    print(f"batch need16 {need16} need32 {need32} cap {cap}")
    assert cap < need32
    want = batch_expected(kind)
    comp = context(SZ4_TEST_ALLOC_CAP=cap)
    try:
        comp.set_batch_chunk(64 * MiB)
        rc, res, msg = attempt(lambda: batch_call(comp, kind, tiled_device(64)))
        mem = comp.debug_memory()
        print(f"{kind}: status {rc} {msg!r} {mem}")
        assert rc == OK, msg
        raw, off = res
        assert off == [sum(len(w) for w in want[:i]) for i in range(65)]
        for i in range(64):
            assert raw[off[i]:off[i + 1]] == want[i], f"item {i}"
        assert comp.last_block_sizes(64) == [len(w) for w in want]
        assert mem["retries"] >= 1 and mem["min_piece"] == 16 * MiB
        assert comp.device_bytes() <= cap
        assert comp.last_error() == ""
    finally:
        comp.close()


# the default piece follows the device's free memory; the cases that count on a retry of a default piece fix the figure
SIZING = {"SZ4_TEST_FREE_BYTES": 64 << 30}
MIXED = (1000, 70001, 65536, 200003, 0, 30000, 65542, 4097)  # below and above the finders' LDS window (65541)


@functools.lru_cache(maxsize=None)
def mixed_case():
    data = synth.enwik8_like(sum(MIXED), seed=93)
    items, at = [], 0
    for n in MIXED:
        items.append(data[at:at + n])
        at += n
    return tuple(items), tuple(pyoracle.oz_block(x, 65535) if x else b"" for x in items)


def test_batch_retry_in_the_second_run_of_a_mixed_piece():
    """A piece with items of both finder kinds runs twice into batchTmp, and k_batch_move puts the blocks in
    caller order.  The failure is the last growth of the second run (the call's last but one: the move table
    follows): the piece is run again from its first item, and the first run's blocks are not taken twice."""
    items, want = mixed_case()
    small = context(**SIZING)
    whole = context(**SIZING)
    try:
        few = [x for x in items if len(x) <= 65541]
        assert succeed(lambda: small.compress_batch(few)) == [w for x, w in zip(items, want) if len(x) <= 65541]
        g_small = small.debug_memory()["growths"]
        assert succeed(lambda: whole.compress_batch(list(items))) == list(want)
        g = whole.debug_memory()["growths"]
    finally:
        small.close()
        whole.close()
    k = g - 1
    assert k > g_small + 1  # past batchTmp and everything the first run grows
    comp = context(SZ4_TEST_FAIL_RESERVE=k, **SIZING)
    try:
        rc, got, msg = attempt(lambda: comp.compress_batch(list(items)))
        assert rc == OK, msg
        assert got == list(want)
        assert comp.last_block_sizes(len(items)) == [len(w) for w in want]
        mem = comp.debug_memory()
        assert mem["injected"] == 1 and mem["retries"] >= 1
        assert comp.last_error() == ""
    finally:
        comp.close()


def test_batch_item_larger_than_the_piece_runs_alone():
    """Halving stops at 16 MiB and an item is at most 4 MiB, so only an explicit piece is smaller than an item:
    the item is then a piece of its own."""
    big = synth.enwik8_like(1_500_000, seed=94)
    items = [tile()[0][:1000], big, tile()[0][5000:305000]]
    comp = context()
    try:
        comp.set_batch_chunk(MiB)
        rc, got, msg = attempt(lambda: comp.compress_batch(items))
        assert rc == OK, msg
        assert got == [pyoracle.oz_block(x, 65535) for x in items]
        assert comp.debug_memory()["retries"] == 0
    finally:
        comp.close()


# ---- d. the floor --------------------------------------------------------------------------------------------
def test_blocks_fail_cleanly_at_the_floor():
    """A device that cannot hold a 16 MiB piece: SZ4_E_NOMEM with a message after two halvings, not a byte
    written (no piece finished), everything released by trim, and the context good for what does fit."""
    import torch
    need16, _ = blocks_needs()
    cap_bytes = need16 // 2
    comp = context(SZ4_TEST_ALLOC_CAP=cap_bytes)
    try:
        comp.set_batch_chunk(64 * MiB)
        src = tiled_device(64)
        out_cap = int(comp._lib.sz4_bound(src.numel(), 65536))
        out = torch.full((out_cap,), 0xA5, dtype=torch.uint8, device="cuda:0")
        rc, _, msg = attempt(lambda: comp.compress_blocks_device(src.data_ptr(), src.numel(), out.data_ptr(), out_cap, 65536, 65535))
        assert rc == NOMEM
        assert msg and comp.last_error() == msg
        mem = comp.debug_memory()
        assert mem["retries"] == 2
        torch.cuda.synchronize()
        assert bool((out == 0xA5).all())
        assert comp.device_bytes() <= cap_bytes
        comp.trim()
        assert comp.device_bytes() == 0
        rc, frame, msg = attempt(lambda: comp.compress_blocks(tiled_device(1), 65536, 65535))
        assert rc == OK, msg
        assert frame == tiled_frame(1) and comp.last_error() == ""
    finally:
        comp.close()


# ---- e. the free-memory cap of the piece sizing ------------------------------------------------------------
def test_piece_sizing_follows_free_memory():
    """A quarter of the free memory over 50 bytes per piece byte: 200 x 24 MiB free gives 24 MiB pieces, so
    40 MiB run as two equal pieces of 20 MiB; an explicit piece size ignores the figure."""
    comp = context(SZ4_TEST_FREE_BYTES=200 * (24 * MiB))
    try:
        assert succeed(lambda: comp.compress_blocks(tiled_device(40), 65536, 65535)) == tiled_frame(40)
        assert comp.last_block_sizes(1024) == tiled_sizes(40)
        mem = comp.debug_memory()
        assert mem["min_piece"] == 20 * MiB and mem["retries"] == 0 and mem["injected"] == 0
        comp.set_batch_chunk(64 * MiB)
        assert succeed(lambda: comp.compress_blocks(tiled_device(40), 65536, 65535)) == tiled_frame(40)
        mem = comp.debug_memory()
        assert mem["min_piece"] == 40 * MiB and mem["retries"] == 0
    finally:
        comp.close()


# ---- f. a failed reservation at every growth of every kind of call ---------------------------------------
def sweep(call, want, env=None, queue=False):
    """Counts the growths G of `call` on a context new to it, then fails growth k on a fresh context for every k
    in 1 .. G.  Either outcome -- SZ4_E_NOMEM with a message, or the oracle's bytes through a fallback -- leaves
    the accounting consistent and the context good for the same call again."""
    env = env or {}
    base = context(**env)
    try:
        assert succeed(lambda: call(base)) == want
        total = base.debug_memory()["growths"]
        assert base.debug_memory()["injected"] == 0
    finally:
        base.close()
    assert total >= 1
    outcomes = {}
    for k in range(1, total + 1):
        comp = context(SZ4_TEST_FAIL_RESERVE=k, **env)
        try:
            before = comp.device_bytes()
            rc, got, msg = attempt(lambda: call(comp))
            if rc == NOMEM:
                assert msg, k
                if queue:  # "nothing left allocated"
                    assert comp.device_bytes() == before, k
            else:
                assert got == want, k
                assert comp.last_error() == "", k
            outcomes[k] = rc
            assert comp.debug_memory()["injected"] == 1, k
            comp.trim()
            assert comp.device_bytes() == 0, k
            rc, got, msg = attempt(lambda: call(comp))
            assert rc == OK, (k, msg)
            assert got == want, k
            assert comp.last_error() == "", k
            assert comp.debug_memory()["injected"] == 1, k
        finally:
            comp.close()
    print(f"{total} growths; recovered at {[k for k, rc in outcomes.items() if rc == OK]}")
    return outcomes


@functools.lru_cache(maxsize=None)
def small_blocks(chain):
    data = synth.enwik8_like(3 * 65536 + 1, seed=95)
    frame = HEADER + b"".join(pyoracle.oz_block(data[o:o + 65536], chain) for o in range(0, len(data), 65536)) + b"\0\0\0\0"
    return data, frame


@pytest.mark.parametrize("chain", [65535, 3])
def test_sweep_compress_blocks(chain):
    data, frame = small_blocks(chain)
    out = sweep(lambda c: c.compress_blocks(data, 65536, chain), frame)
    assert set(out.values()) == {NOMEM}  # one piece, below the floor: nothing to fall back to


@functools.lru_cache(maxsize=None)
def filtered_case():
    sizes = (0, 1, 15, 4097, 65536, 65542, 70001, 1000, 33333, 8191, 24, 40000)
    elems = (1, 2, 4, 8, 1, 2, 4, 8, 2, 4, 8, 1)
    filters = tuple(BITS if i % 2 else BYTES for i in range(len(sizes)))
    text = synth.enwik8_like(80_000, seed=96)
    w = np.random.default_rng(97).normal(0, 0.02, 40_000)
    pay = {1: text, 2: (w.astype(np.float32).view(np.uint32) >> 16).astype(np.uint16).tobytes(),
           4: w.astype(np.float32).tobytes(), 8: w.astype(np.float64).tobytes()}
    items = tuple(pay[e][:n] for n, e in zip(sizes, elems))
    want = tuple(pyoracle.oz_block(planes.bit_split(x, e) if f == BITS else planes.split(x, e), 65535) if x else b""
                 for x, e, f in zip(items, elems, filters))
    return items, elems, filters, want


def test_sweep_compress_batch_filtered():
    items, elems, filters, want = filtered_case()
    names = ["bits" if f == BITS else "bytes" for f in filters]
    out = sweep(lambda c: c.compress_batch_typed(list(items), list(elems), 65535, filters=names), list(want), env=SIZING)
    assert set(out.values()) == {OK}  # several items: the piece is tried again (the failure does not come twice)


def test_sweep_stream_two_chunks():
    data = synth.enwik8_like(9 * MiB, seed=98)
    want = pyoracle.oz_lz4(data, 3)

    def call(c):
        c.set_stream_chunk(8 * MiB)
        return c.lz4(data, 3)

    sweep(call, want)


@pytest.mark.parametrize("chain", [3, 65535])
def test_sweep_stream_with_dictionary(chain):
    data = synth.enwik8_like(2 * MiB + 70000, seed=99)
    body, dictionary = data[:2 * MiB], data[-70000:]
    want = pyoracle.oz_lz4(body, chain, dictionary)
    sweep(lambda c: c.lz4(body, chain, dictionary), want)


@pytest.mark.parametrize("split", [False, True])
def test_sweep_unlz4(split):
    """The decoder block by block, and in split mode (whose scratch falls back to block by block)."""
    data, frame = small_blocks(65535)
    sweep(lambda c: c.unlz4(frame), data, env={"SZ4_UNLZ4_SPLIT": 1} if split else None)


def test_sweep_unlz4_batch_typed():
    items, elems, _, _ = filtered_case()
    blocks = [pyoracle.oz_block(planes.split(x, e), 3) if x else b"" for x, e in zip(items, elems)]
    sweep(lambda c: c.unlz4_batch_typed(blocks, list(elems)), list(items))


def test_sweep_decode_queue_creation():
    import torch
    items = [tile()[0][:70001], tile()[0][100000:100900]]
    blocks = [pyoracle.oz_block(x, 65535) for x in items]

    def call(c):
        q = c.decode_queue(16, MiB)
        try:
            dev = "cuda:0"
            src = on_device(b"".join(blocks))
            dst = torch.zeros(sum(map(len, items)), dtype=torch.uint8, device=dev)
            sp, dp, at, to = [], [], src.data_ptr(), dst.data_ptr()
            for b, x in zip(blocks, items):
                sp.append(at)
                dp.append(to)
                at += len(b)
                to += len(x)
            t64 = lambda v: torch.tensor(v, dtype=torch.int64).to(dev)
            t32 = lambda v: torch.tensor(v, dtype=torch.int32).to(dev)
            sizes, status = torch.zeros(2, dtype=torch.int32, device=dev), torch.full((2,), -7, dtype=torch.int32, device=dev)
            q.enqueue(t64(sp), t32([len(b) for b in blocks]), t64(dp), t32([len(x) for x in items]), sizes, status)
            torch.cuda.synchronize()
            return dst.cpu().numpy().tobytes(), sizes.tolist(), status.tolist()
        finally:
            q.close()

    out = sweep(call, (b"".join(items), [len(x) for x in items], [0, 0]), queue=True)
    assert set(out.values()) == {NOMEM}


def test_sweep_compress_queue_creation():
    import torch
    items, want = (tuple(v for v in part if v) for part in mixed_case())

    def call(c):
        q = c.compress_queue([len(x) for x in items])
        try:
            dev = "cuda:0"
            t = on_device(b"".join(items))
            out = torch.zeros(q.bound, dtype=torch.uint8, device=dev)
            ptrs = torch.zeros(q.count, dtype=torch.int64, device=dev)
            sizes = torch.zeros(q.count, dtype=torch.int32, device=dev)
            status = torch.full((q.count,), -7, dtype=torch.int32, device=dev)
            total = torch.zeros(1, dtype=torch.int64, device=dev)
            q.enqueue(q.tensor_tables(t), out, ptrs, sizes, status, total)
            torch.cuda.synchronize()
            return out[:int(total.item())].cpu().numpy().tobytes(), sizes.tolist(), status.tolist()
        finally:
            q.close()

    out = sweep(call, (b"".join(want), [len(w) for w in want], [0] * len(want)), queue=True)
    assert set(out.values()) == {NOMEM}
