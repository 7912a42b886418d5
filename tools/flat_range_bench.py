#!/usr/bin/env python
"""What FlatIndex.range_search costs at a SIFT1M-like shape, through the public API, against what answers the same
question today.

Per batch size, every leg interleaved in one process (HIP-event timed, median and max - min over the steps):
  fused_k100      FlatIndex.search(k=100), use_fused_search = True (tpq_flat_topk: one pass over the same tiles)
  range_hits10 / range_hits100 / range_hits1000
                  FlatIndex.range_search at the median 10th / 100th / 1000th value of one search: count, prefix sum,
                  sync, fill
  range_inf       threshold +inf: the count pass, the prefix sum and the host sync alone
  matrix_hits100  what a user does without it: the default route's [n_query, capacity] matrix, >= and nonzero (only
                  while the matrix stays below --matrix-limit-gb), with the allocator's high-water mark
  ivfflat_hits100 IVFFlatIndex.range_search with every cell probed (only up to --ivf-max-nq queries)
Prints one JSON line and writes it to --out.

    python tools/flat_range_bench.py [--n 1000000 --nq 1,100,1000,10000 --steps 10 --warmup 2]
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

from flat_bench import peak_temporary_bytes, timed  # noqa: E402  (tools/ is the script's own directory)

FP32_MATRIX_PEAK_TFLOPS = 155.0


def stats(ms, nq):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "spread_ms": round(float(ms.max() - ms.min()), 4),
            "queries_per_s": round(nq / (float(np.median(ms)) * 1e-3), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", default="1,100,1000,10000")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--n-cells", type=int, default=256)
    ap.add_argument("--ivf-max-nq", type=int, default=1000)
    ap.add_argument("--matrix-limit-gb", type=float, default=8.0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_range_bench.json"))
    args = ap.parse_args()

    from torchpq_amd import metric
    from torchpq_amd.index import FlatIndex, IVFFlatIndex

    assert torch.cuda.is_available(), "flat_range_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    centers = torch.randn(args.d, 256, device="cuda", generator=gen) * 4
    pick = torch.randint(0, 256, (args.n,), device="cuda", generator=gen)
    base = (centers[:, pick] + torch.randn(args.d, args.n, device="cuda", generator=gen)).contiguous()
    flat = FlatIndex(args.d, initial_size=args.n)
    np.random.seed(0)
    torch.manual_seed(0)
    ivf = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=2 * args.n // args.n_cells)
    ivf.train(base[:, :min(args.n, 100000)].contiguous())
    for b0 in range(0, args.n, 250000):
        flat.add(base[:, b0:b0 + 250000].contiguous())
        ivf.add(base[:, b0:b0 + 250000].contiguous())
    ivf.n_probe = ivf.n_cells
    ivf.use_smart_probing = False
    sizes = [int(s) for s in args.nq.split(",")]
    all_queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:max(sizes)]]
                   + 0.3 * torch.randn(args.d, max(sizes), device="cuda", generator=gen)).contiguous()
    del base, centers, pick

    def fused(queries, k):
        flat.use_fused_search = True
        try:
            return flat.search(queries, k=k)
        finally:
            flat.use_fused_search = False

    def by_matrix(queries, thr):
        sims = metric.negative_squared_l2_distance(queries, flat._storage.view(args.d, -1))
        sims = sims.masked_fill((flat._address2id < 0)[None, :], float("-inf"))
        hit = torch.nonzero(sims >= thr)
        return hit, sims[hit[:, 0], hit[:, 1]]

    ranks = (10, 100, 1000)
    probe = fused(all_queries[:, :min(1000, max(sizes))].contiguous(), max(ranks))[0]
    thresholds = {f"hits{r}": float(probe[:, r - 1].median()) for r in ranks}
    thresholds["inf"] = float("inf")
    del probe
    result = {"tool": "flat_range_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "steps": args.steps, "warmup": args.warmup, "n_cells": args.n_cells,
              "fp32_matrix_peak_tflops": FP32_MATRIX_PEAK_TFLOPS, "thresholds": thresholds, "batches": []}
    for nq in sizes:
        queries = all_queries[:, :nq].contiguous()
        legs = {"fused_k100": lambda: fused(queries, 100)}
        for name, thr in thresholds.items():
            legs["range_" + name] = lambda thr=thr: flat.range_search(queries, thr)
        if nq * args.n * 4 <= args.matrix_limit_gb * 2 ** 30:
            legs["matrix_hits100"] = lambda: by_matrix(queries, thresholds["hits100"])
        if nq <= args.ivf_max_nq:
            legs["ivfflat_hits100"] = lambda: ivf.range_search(queries, thresholds["hits100"])
        events = {name: [] for name in legs}
        out = {}
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():          # interleaved: every leg sees the same clocks
                ev, out[name] = timed(fn)
                if step >= args.warmup:
                    events[name].append(ev)
        torch.cuda.synchronize()
        row = {"nq": nq, "n_parts": flat._flat_range.last_n_parts, "fused_n_parts": flat._flat_topk.last_n_parts}
        for name, evs in events.items():
            row[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
            if name.startswith("range_") or name == "ivfflat_hits100":
                row[name]["hits_per_query"] = round(int(out[name][0][-1]) / nq, 2)
                row[name]["over_fused_k100"] = round(row[name]["median_ms"] / row["fused_k100"]["median_ms"], 4)
        if "matrix_hits100" in legs:
            row["matrix_hits100"]["hits_per_query"] = round(out["matrix_hits100"][0].shape[0] / nq, 2)
            row["matrix_hits100"]["over_range_hits100"] = round(
                row["matrix_hits100"]["median_ms"] / row["range_hits100"]["median_ms"], 4)
        row["count_pass_tflops"] = round(2.0 * args.d * args.n * nq / (row["range_inf"]["median_ms"] * 1e-3) / 1e12, 2)
        del out
        for name in ("range_hits100", "range_hits1000", "matrix_hits100"):
            if name in legs:
                row[name]["peak_temporary_bytes"] = peak_temporary_bytes(legs[name])
        result["batches"].append(row)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
