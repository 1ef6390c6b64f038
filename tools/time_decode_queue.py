#!/usr/bin/env python3
"""Times the decode queue next to the synchronous batch decoders, in one process.

Plain: time_batch.py's leg (b) -- 100 MB of enwik8-shaped text as 64 KiB items at -9 -- decoded in batches of
the first 1, 8, 64 and 1526 items three ways:
  (i)   sz4_unlz4_batch_device (host tables, two stream waits): the baseline of the same run
  (ii)  sz4_dq_enqueue on device tables, then one stream wait
  (iii) replay of a graph captured from that enqueue, then one stream wait
Typed: the same at widths 2, 4 and 8 on time_batch.py --elem's data (increasing int32 counters, 1526 items of
64 KiB) at chain 3, (i) being sz4_unlz4_batch_typed_device.
Every figure is host time around call plus stream synchronisation: one warm-up and --reps timed calls per
leg, the whole sequence --rounds times; mean [min .. max] in milliseconds over all timed calls.  The C
functions are called on prebuilt argument arrays, so no leg pays for Python marshalling.
    python3 tools/time_decode_queue.py [--mb 100] [--reps 5] [--rounds 2]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import smallz4_amd  # noqa: E402
from smallz4_amd import synth  # noqa: E402

ITEM = 65536
BATCHES = (1, 8, 64, 1526)


def legs(comp, queue, t_in, blocks, off, elem, a, label):
    """Times the three ways on the first B items of `blocks` (offsets `off`) for every B, checking each result."""
    dev = t_in.device
    lib, h = comp._lib, comp._h
    n_items = len(off) - 1
    dec = torch.empty(t_in.numel(), dtype=torch.uint8, device=dev)
    sizes = [min(ITEM, t_in.numel() - k * ITEM) for k in range(n_items)]
    src = torch.tensor([blocks.data_ptr() + off[k] for k in range(n_items)], dtype=torch.int64).to(dev)
    ssz = torch.tensor([off[k + 1] - off[k] for k in range(n_items)], dtype=torch.int32).to(dev)
    dst = torch.tensor([dec.data_ptr() + k * ITEM for k in range(n_items)], dtype=torch.int64).to(dev)
    cap = torch.tensor(sizes, dtype=torch.int32).to(dev)
    el = None if elem == 1 else torch.full((n_items,), elem, dtype=torch.uint8, device=dev)
    osz = torch.zeros(n_items, dtype=torch.int32, device=dev)
    st = torch.zeros(n_items, dtype=torch.int32, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for B in BATCHES:
        B = min(B, n_items)
        total = sum(sizes[:B])
        c_off = (ctypes.c_uint64 * (B + 1))(*off[:B + 1])
        c_res = (ctypes.c_uint64 * (B + 1))()
        c_el = (ctypes.c_uint8 * B)(*([elem] * B))

        def sync_call():
            if elem == 1:
                rc = lib.sz4_unlz4_batch_device(h, ctypes.c_void_p(blocks.data_ptr()), c_off, B, ctypes.c_void_p(dec.data_ptr()),
                                                total, c_res, ctypes.c_void_p(stream))
            else:
                rc = lib.sz4_unlz4_batch_typed_device(h, ctypes.c_void_p(blocks.data_ptr()), c_off, c_el, B,
                                                      ctypes.c_void_p(dec.data_ptr()), total, c_res, ctypes.c_void_p(stream))
            assert rc == 0 and c_res[B] == total, rc

        def enqueue():
            queue.enqueue(src, ssz, dst, cap, osz, st, elems=el, count=B)
            torch.cuda.synchronize()

        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            queue.enqueue(src, ssz, dst, cap, osz, st, elems=el, count=B)

        def replay():
            graph.replay()
            torch.cuda.synchronize()

        ways = {"(i) synchronous": sync_call, "(ii) enqueue": enqueue, "(iii) graph replay": replay}
        times = {k: [] for k in ways}
        for _ in range(a.rounds):
            for name, fn in ways.items():
                for rep in range(a.reps + 1):
                    dec[:total].zero_()
                    st.fill_(-1)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    assert torch.equal(dec[:total], t_in[:total]), (label, B, name)
                    if name[1:3] != "i)":
                        assert not bool(st[:B].any()), (label, B, name)
                    if rep:
                        times[name].append(dt * 1e3)
        del graph
        row = ", ".join(f"{name} {sum(ts) / len(ts):.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]" for name, ts in times.items())
        print(f"{label}, {B} items ({total} bytes): {row}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    comp = smallz4_amd.Compressor()
    n = int(a.mb * 1e6)
    queue = comp.decode_queue((n + ITEM - 1) // ITEM, n + n // 64 + 4096)

    def pieces(t):
        sizes = [min(ITEM, t.numel() - o) for o in range(0, t.numel(), ITEM)]
        return [t.data_ptr() + k * ITEM for k in range(len(sizes))], sizes

    t_in = torch.frombuffer(bytearray(synth.enwik8_like(n, seed=8)), dtype=torch.uint8).to(dev)
    ptrs, sizes = pieces(t_in)
    bound = comp.batch_bound(sizes) + 64
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    off = comp.compress_batch_device(ptrs, sizes, out.data_ptr(), bound, 65535)
    legs(comp, queue, t_in, out[:off[-1]].clone(), off, 1, a, "text at -9, width 1")

    m = 1526 * ITEM
    g = np.random.default_rng(9)
    data = (np.cumsum(g.integers(0, 70000, m // 4 + 1)) & 0x7FFFFFFF).astype(np.int32).tobytes()[:m]
    t_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    ptrs, sizes = pieces(t_in)
    bound = comp.batch_bound(sizes) + 64
    out = torch.empty(bound, dtype=torch.uint8, device=dev)
    for E in (2, 4, 8):
        off = comp.compress_batch_typed_device(ptrs, sizes, [E] * len(sizes), out.data_ptr(), bound, 3)
        legs(comp, queue, t_in, out[:off[-1]].clone(), off, E, a, f"int32 counters at chain 3, width {E}")
    queue.close()


if __name__ == "__main__":
    main()
