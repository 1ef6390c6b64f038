#!/usr/bin/env python3
"""Times the ragged batch API on configs[1]'s input (100 MB of enwik8-shaped text) at -9, in one process:
  (a) compress_blocks_device, 64 KiB blocks                       -- the yardstick
  (b) compress_batch_device over the same bytes as separate 64 KiB device pointers
  (c) compress_batch_device over the same bytes cut into sizes drawn from 1 KiB..256 KiB (fixed seed)
then decodes (b)'s blocks with unlz4_batch_device next to unlz4_device on the equivalent frame.  Each leg
runs one warm-up and --reps timed calls in a row (so (a) keeps its cached plan, as in bench.py), and the
whole sequence runs --rounds times so that drift shows; rates are means over all timed calls with the
min..max spread, the stage split and the gather time are the last call's.  The batch legs' times include
the Python binding's marshalling of the pointer and size lists.
    python3 tools/time_batch.py [--mb 100] [--reps 5] [--rounds 2] [--chain 65535]
With --elem 2,4,8 it times the typed batch API's two kernels instead (see typed() below); with --filter bits
beside it, the bit-plane shuffle's gather and merge (the filtered calls, every item SZ4_FILTER_BITS)."""
import argparse
import os
import random
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import smallz4_amd  # noqa: E402
from smallz4_amd import synth  # noqa: E402


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]) / 2


def typed(a):
    """--elem: the split gather (k_batch_gather_planes) against the plain gather on the same items, and the
    merge (k_batch_merge) against a device-to-device copy of the same bytes.  Item sets: 1526 items of
    64 KiB, 10 000 items of 200 bytes to 4 KiB, and those cut down to whole elements; medians of the device
    times over reps x rounds calls.  --filter bits: the same loop through the filtered calls, every item (width 1
    too) shuffled into its bit planes (k_batch_gather_bits, k_batch_merge_bits); the plain gather stays the base."""
    import numpy as np
    dev = torch.device("cuda:0")
    widths = [1] + [int(x) for x in a.elem.split(",") if int(x) != 1]
    bits = a.filter == "bits"
    rng = random.Random(9)
    small = [rng.randrange(200, 4097) for _ in range(10000)]
    # the third set is the second with whole elements only: every item then lands at a multiple of its width
    sets = {"1526 x 64 KiB": [65536] * 1526, "10000 x 200 B..4 KiB": small,
            "10000 x 200 B..4 KiB, multiples of 8": [k & ~7 for k in small]}
    comp = smallz4_amd.Compressor()
    comp.set_timing(True)
    for label, sizes in sets.items():
        n = sum(sizes)
        g = np.random.default_rng(9)
        data = (np.cumsum(g.integers(0, 70000, n // 4 + 1)) & 0x7FFFFFFF).astype(np.int32).tobytes()[:n]
        t_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
        ptrs, at = [], 0
        for k in sizes:
            ptrs.append(t_in.data_ptr() + at)
            at += k
        cap = comp.batch_bound(sizes) + 64
        out = torch.empty(cap, dtype=torch.uint8, device=dev)
        dec = torch.empty(n, dtype=torch.uint8, device=dev)
        dup = torch.empty(n, dtype=torch.uint8, device=dev)
        copies = []
        for _ in range(a.reps * a.rounds + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dup.copy_(t_in)
            e1.record()
            torch.cuda.synchronize()
            copies.append(e0.elapsed_time(e1))
        copy_ms = median(copies[1:])
        print(f"{label}: {n} bytes, device-to-device copy {copy_ms:.4f} ms [{min(copies[1:]):.4f} .. {max(copies[1:]):.4f}]",
              flush=True)
        base = None
        for E in ([0] if bits else []) + widths:  # width 0: the plain gather, the base of a --filter bits run
            elems = [E or 1] * len(sizes)
            filters = [smallz4_amd.FILTERS["bits" if bits and E else "bytes"]] * len(sizes)
            gather, merge = [], []
            for rep in range(a.reps * a.rounds + 1):
                off = comp.compress_batch_filtered_device(ptrs, sizes, elems, filters, out.data_ptr(), cap, a.chain)
                g_ms = comp.last_gather_ms()
                got = comp.unlz4_batch_filtered_device(out.data_ptr(), off, elems, filters, dec.data_ptr(), n)
                m_ms = comp.last_merge_ms()
                assert got[-1] == n and torch.equal(dec, t_in), (label, E)
                if rep:
                    gather.append(g_ms)
                    merge.append(m_ms)
            g_ms, m_ms = median(gather), median(merge)
            base = g_ms if E == (0 if bits else 1) else base
            if not E:
                print(f"  plain gather {g_ms:.4f} ms [{min(gather):.4f} .. {max(gather):.4f}]", flush=True)
                continue
            line = (f"  E={E}{' bits' if bits else ''}: gather {g_ms:.4f} ms [{min(gather):.4f} .. {max(gather):.4f}] ({g_ms / base:.2f}x the plain "
                    f"gather), {off[-1]} bytes out")
            if E > 1 or bits:
                line += f", merge {m_ms:.4f} ms [{min(merge):.4f} .. {max(merge):.4f}] ({m_ms / copy_ms:.2f}x the copy)"
            print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mb", type=float, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--chain", type=int, default=65535)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--elem", default="", help="element widths, e.g. 2,4,8: time the typed gather and merge instead")
    ap.add_argument("--filter", default="bytes", choices=["bytes", "bits"],
                    help="with --elem: bits times the bit-plane shuffle's gather and merge")
    a = ap.parse_args()
    if a.elem:
        return typed(a)
    n = int(a.mb * 1e6)
    data = synth.enwik8_like(n, seed=8)
    dev = torch.device("cuda:0")
    t_in = torch.frombuffer(bytearray(data), dtype=torch.uint8).to(dev)
    base = t_in.data_ptr()
    uniform = [min(65536, n - o) for o in range(0, n, 65536)]
    rng = random.Random(8)
    ragged, left = [], n
    while left:
        k = min(left, rng.randrange(1 << 10, (256 << 10) + 1))
        ragged.append(k)
        left -= k

    def ptrs(sizes):
        out, at = [], 0
        for k in sizes:
            out.append(base + at)
            at += k
        return out

    comp = smallz4_amd.Compressor()
    comp.set_timing(True)
    cap = max(comp.batch_bound(ragged), comp.batch_bound(uniform)) + 64
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    p_uniform, p_ragged = ptrs(uniform), ptrs(ragged)
    legs = {
        "a blocks 64K": lambda: comp.compress_blocks_device(base, n, out.data_ptr(), cap, 65536, a.chain, "none"),
        "b batch 64K": lambda: comp.compress_batch_device(p_uniform, uniform, out.data_ptr(), cap, a.chain)[-1],
        "c batch ragged": lambda: comp.compress_batch_device(p_ragged, ragged, out.data_ptr(), cap, a.chain)[-1],
    }
    times = {k: [] for k in legs}
    info = {}
    for _ in range(a.rounds):
        for name, fn in legs.items():
            for rep in range(a.reps + 1):  # repetition 0 warms the leg's shapes up (and plans: (a) caches its plan)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                size = fn()  # returns after its stream has finished
                dt = time.perf_counter() - t0
                if rep:
                    times[name].append(dt)
            info[name] = (size, {k: round(v, 3) for k, v in comp.last_stage_ms().items()},
                          round(comp.last_gather_ms(), 3) if name[0] != "a" else None)
    for name, ts in times.items():
        rates = sorted(n / t / 1e6 for t in ts)
        size, st, gather = info[name]
        items = {"a": len(uniform), "b": len(uniform), "c": len(ragged)}[name[0]]
        print(f"{name}: {n / (sum(ts) / len(ts)) / 1e6:.0f} MB/s (min {rates[0]:.0f}, max {rates[-1]:.0f} over {len(ts)}), "
              f"{items} items, {size} bytes out, stages {st}" + (f", gather {gather} ms" if gather is not None else ""),
              flush=True)

    # decode: (b)'s bare blocks item by item, and the same blocks as one frame
    off = comp.compress_batch_device(p_uniform, uniform, out.data_ptr(), cap, a.chain)
    blocks = out[:off[-1]].clone()
    frame_cap = n + n // 8 + (1 << 20)
    frame = torch.empty(frame_cap, dtype=torch.uint8, device=dev)
    flen = comp.compress_blocks_device(base, n, frame.data_ptr(), frame_cap, 65536, a.chain)
    dec = torch.empty(n, dtype=torch.uint8, device=dev)
    dlegs = {
        "unlz4_batch_device": lambda: comp.unlz4_batch_device(blocks.data_ptr(), off, dec.data_ptr(), n)[-1],
        "unlz4_device (frame)": lambda: comp.unlz4_device(frame.data_ptr(), flen, dec.data_ptr(), n),
    }
    dtimes = {k: [] for k in dlegs}
    for _ in range(a.rounds):
        for name, fn in dlegs.items():
            for rep in range(a.reps + 1):
                dec.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                dt = time.perf_counter() - t0
                assert got == n and torch.equal(dec, t_in), name
                if rep:
                    dtimes[name].append(dt)
    for name, ts in dtimes.items():
        rates = sorted(n / t / 1e6 for t in ts)
        print(f"{name}: {n / (sum(ts) / len(ts)) / 1e6:.0f} MB/s decoded (min {rates[0]:.0f}, max {rates[-1]:.0f} over {len(ts)})",
              flush=True)


if __name__ == "__main__":
    main()
