#!/usr/bin/env python3
"""Times the compress queue next to the synchronous batch compressor, in one process.

The first 1, 8, 64 and 1526 items of 64 KiB of enwik8-shaped text (time_batch.py's leg (b)) at -9, compressed
three ways:
  (i)   sz4_compress_batch_device (plans, reserves, uploads and waits on every call): the baseline of the same run
  (ii)  sz4_cq_enqueue on a queue created for these sizes, then one stream wait
  (iii) replay of a graph captured from that enqueue, then one stream wait
Every result is compared byte for byte with (i)'s.  Every figure is host time around call plus stream
synchronisation: one warm-up and --reps timed calls per leg, the legs in turn, the whole sequence --rounds
times; mean [min .. max] in milliseconds over all timed calls.  The C functions are called on prebuilt argument
arrays, so no leg pays for Python marshalling.  The queue's held scratch (sz4_device_bytes after create minus
before) is printed with every row.
--sized times a sized queue (sz4_cq_create_sized) with the same capacities next to them, at 64 and 1526 items:
  (iv)  sz4_cq_enqueue_sized with every size equal to its capacity, then one stream wait: (ii) plus k_cq_plan
  (v)   replay of a graph captured from that enqueue
  (vi)  the same enqueue with every size a quarter of its capacity: what the capacity-sized grids cost when
        the sizes are small (compared byte for byte with a synchronous call on the quarter sizes)
    python3 tools/time_compress_queue.py [--reps 3] [--rounds 2] [--sized]"""
import argparse
import ctypes
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import smallz4_amd  # noqa: E402
from smallz4_amd import synth  # noqa: E402

ITEM = 65536
BATCHES = (1, 8, 64, 1526)
CHAIN = 65535


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--sized", action="store_true", help="add the sized queue's legs (64 and 1526 items only)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    comp = smallz4_amd.Compressor()
    lib, h = comp._lib, comp._h
    n = max(BATCHES) * ITEM
    t_in = torch.frombuffer(bytearray(synth.enwik8_like(n, seed=8)), dtype=torch.uint8).to(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for B in (BATCHES[2:] if a.sized else BATCHES):
        sizes = [ITEM] * B
        bound = comp.batch_bound(sizes)
        ref = torch.empty(bound, dtype=torch.uint8, device=dev)
        out = torch.empty(bound, dtype=torch.uint8, device=dev)
        c_ptrs = (ctypes.c_void_p * B)(*[t_in.data_ptr() + k * ITEM for k in range(B)])
        c_sizes = (ctypes.c_uint32 * B)(*sizes)
        c_off = (ctypes.c_uint64 * (B + 1))()

        def sync_call(target=out):
            rc = lib.sz4_compress_batch_device(h, c_ptrs, c_sizes, B, CHAIN, ctypes.c_void_p(target.data_ptr()), bound, c_off,
                                               ctypes.c_void_p(stream))
            assert rc == 0, rc

        sync_call(ref)
        off = list(c_off)
        before = comp.device_bytes()
        queue = comp.compress_queue(sizes, None, CHAIN)
        held = comp.device_bytes() - before
        src = torch.tensor(list(c_ptrs), dtype=torch.int64).to(dev)
        ptrs = torch.zeros(B, dtype=torch.int64, device=dev)
        bsz = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.zeros(B, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)

        def enqueue():
            queue.enqueue(src, out, ptrs, bsz, st, total)
            torch.cuda.synchronize()

        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            queue.enqueue(src, out, ptrs, bsz, st, total)

        def replay():
            graph.replay()
            torch.cuda.synchronize()

        ways = {"(i) synchronous": sync_call, "(ii) enqueue": enqueue, "(iii) graph replay": replay}
        refs = {}
        if a.sized:
            # the quarter sizes' expected bytes, from the synchronous call
            quarter = [ITEM // 4] * B
            q_sizes = (ctypes.c_uint32 * B)(*quarter)
            q_off = (ctypes.c_uint64 * (B + 1))()
            ref4 = torch.empty(bound, dtype=torch.uint8, device=dev)
            rc = lib.sz4_compress_batch_device(h, c_ptrs, q_sizes, B, CHAIN, ctypes.c_void_p(ref4.data_ptr()), bound, q_off,
                                               ctypes.c_void_p(stream))
            assert rc == 0, rc
            before = comp.device_bytes()
            squeue = comp.compress_queue_sized(sizes, None, CHAIN)
            sheld = comp.device_bytes() - before
            nsz = torch.tensor(sizes, dtype=torch.int32).to(dev)
            nsz4 = torch.tensor(quarter, dtype=torch.int32).to(dev)

            def sized_enqueue():
                squeue.enqueue(src, nsz, out, ptrs, bsz, st, total)
                torch.cuda.synchronize()

            def sized_quarter():
                squeue.enqueue(src, nsz4, out, ptrs, bsz, st, total)
                torch.cuda.synchronize()

            torch.cuda.synchronize()
            sgraph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(sgraph):
                squeue.enqueue(src, nsz, out, ptrs, bsz, st, total)

            def sized_replay():
                sgraph.replay()
                torch.cuda.synchronize()

            ways.update({"(iv) sized enqueue": sized_enqueue, "(v) sized graph replay": sized_replay,
                         "(vi) sized enqueue, quarter sizes": sized_quarter})
            refs["(vi) sized enqueue, quarter sizes"] = (ref4, list(q_off))
        times = {k: [] for k in ways}
        for _ in range(a.rounds):
            for name, fn in ways.items():
                for rep in range(a.reps + 1):
                    out.zero_()
                    st.fill_(-1)
                    total.fill_(-1)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn()
                    dt = time.perf_counter() - t0
                    want, woff = refs.get(name, (ref, off))
                    assert torch.equal(out[:woff[-1]], want[:woff[-1]]), (B, name)
                    if name[1:3] != "i)":
                        got = (st.cpu().tolist(), int(total[0]), [p - out.data_ptr() for p in ptrs.cpu().tolist()])
                        assert got == ([0] * B, woff[-1], woff[:-1]), (B, name, rep, got[0][:4], got[1], woff[-1], got[2][:4])
                    if rep:
                        times[name].append(dt * 1e3)
        del graph
        queue.close()
        if a.sized:
            del sgraph
            squeue.close()
            print(f"(the sized queue holds {sheld} bytes)")
        row = ", ".join(f"{name} {sum(ts) / len(ts):.3f} ms [{min(ts):.3f} .. {max(ts):.3f}]" for name, ts in times.items())
        print(f"text at -9, {B} items ({B * ITEM} bytes -> {off[-1]}), queue holds {held} bytes: {row}", flush=True)


if __name__ == "__main__":
    main()
