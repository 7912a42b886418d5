#!/usr/bin/env python
"""What FlatIndex.search costs on its two routes, at a SIFT1M-like shape, through the public API.

Per batch size, both legs interleaved in one process (HIP-event timed, median and spread over the steps):
  (a) default      library GEMM -> [n_query, capacity] matrix -> mask -> row select -> address -> id
  (b) fused        use_fused_search = True: tpq_flat_topk, no matrix
Reported per leg: ms per call, queries/s, the peak temporary memory of one call (allocator high-water mark above what
was held before it); for (b) the flop rate (2 d n nq) against the 155 TF of the fp32 matrix pipe and the parts per
query it chose; the overlap of the two routes' top-k ids (the routes round differently: near-ties may swap).
The yardstick is the default route of the same build.  Prints one JSON line and writes it to --out.

    python tools/flat_bench.py [--n 1000000 --nq 1,100,1000,10000 --k 100 --steps 10 --warmup 2 --out profiles/flat_fused_bench.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP32_MATRIX_PEAK_TFLOPS = 155.0


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return (e0, e1), out


def stats(ms, nq):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4), "queries_per_s": round(nq / (float(np.median(ms)) * 1e-3), 1)}


def peak_temporary_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    held = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - held
    del out
    return int(peak)


def overlap(a, b):
    """mean fraction of the ids of a's rows that b's rows hold too"""
    total = 0.0
    for r0 in range(0, a.shape[0], 1000):
        x, y = a[r0:r0 + 1000], b[r0:r0 + 1000]
        total += float((x[:, :, None] == y[:, None, :]).any(2).float().sum())
    return round(total / a.numel(), 6)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", default="1,100,1000,10000")
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_fused_bench.json"))
    args = ap.parse_args()

    from torchpq_amd.index import FlatIndex

    assert torch.cuda.is_available(), "flat_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    centers = torch.randn(args.d, 256, device="cuda", generator=gen) * 4
    pick = torch.randint(0, 256, (args.n,), device="cuda", generator=gen)
    base = (centers[:, pick] + torch.randn(args.d, args.n, device="cuda", generator=gen)).contiguous()
    flat = FlatIndex(args.d, initial_size=args.n)
    for b0 in range(0, args.n, 250000):
        flat.add(base[:, b0:b0 + 250000].contiguous())
    sizes = [int(s) for s in args.nq.split(",")]
    all_queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:max(sizes)]]
                   + 0.3 * torch.randn(args.d, max(sizes), device="cuda", generator=gen)).contiguous()
    del base, centers, pick

    def search(queries, fused):
        flat.use_fused_search = fused
        try:
            return flat.search(queries, k=args.k)
        finally:
            flat.use_fused_search = False

    result = {"tool": "flat_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n, "k": args.k,
              "steps": args.steps, "warmup": args.warmup, "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS,
              "batches": []}
    for nq in sizes:
        queries = all_queries[:, :nq].contiguous()
        legs = {"default": lambda: search(queries, False), "fused": lambda: search(queries, True)}
        events = {name: [] for name in legs}
        out = {}
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():          # interleaved: both legs see the same clocks
                ev, out[name] = timed(fn)
                if step >= args.warmup:
                    events[name].append(ev)
        torch.cuda.synchronize()
        row = {"nq": nq, "n_parts": flat._flat_topk.last_n_parts}
        for name, evs in events.items():
            row[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
        row["fused_tflops"] = round(2.0 * args.d * args.n * nq / (row["fused"]["median_ms"] * 1e-3) / 1e12, 2)
        row["fused_fraction_of_fp32_matrix_peak"] = round(row["fused_tflops"] / FP32_MATRIX_PEAK_TFLOPS, 4)
        row["fused_over_default_time"] = round(row["fused"]["median_ms"] / row["default"]["median_ms"], 4)
        row["topk_id_overlap"] = overlap(out["fused"][1], out["default"][1])
        del out
        for name, fn in legs.items():
            row[name]["peak_temporary_bytes"] = peak_temporary_bytes(fn)
        result["batches"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
