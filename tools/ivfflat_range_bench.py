#!/usr/bin/env python
"""What IVFFlatIndex.range_search costs next to IVFFlatIndex.search, at the shape of tools/ivfflat_bench.py.

Thresholds: the medians over the queries of the 10th, 100th and 1000th value of one search(k = 1000) -- roughly 10, 100
and 1000 hits per query -- and +inf, which has no hit: the count pass and the host sync alone.
Per step, interleaved in one process (HIP-event timed, median and spread over the steps):
  search_k100        IVFFlatIndex.search(k = 100): the yardstick (coarse step + top-k list scan + address -> id)
  range_hits10 / range_hits100 / range_hits1000 / range_inf    IVFFlatIndex.range_search(threshold)
  kernels_hits*      the two passes alone (IVFFlatRangeHip) on the coarse step's cells
  scan_k100_kernel   the top-k list scan alone (IVFFlatTopkHip) on the same cells
range_search ends with a host sync (the hit count sizes the outputs), so its event pair spans the device work of the
call; the other legs are asynchronous and their pairs span the device work likewise.
Reported: every leg's median / min / max, the ratio of each range leg to search_k100 (two passes over the same bytes
bound it at 2 plus the sync that range_inf isolates) and of each kernels leg to scan_k100_kernel, hits per query.
Prints one JSON line and writes it to --out.

    python tools/ivfflat_range_bench.py [--n 1000000 --nq 10000 --steps 20 --warmup 3 --out profiles/ivfflat_range_bench.json]
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

from tools.ivfflat_bench import clustered, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100, help="k of the yardstick search")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_range_bench.json"))
    args = ap.parse_args()

    from torchpq_amd.index import IVFFlatIndex

    assert torch.cuda.is_available(), "ivfflat_range_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    idx = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=max(64, 2 * args.n // args.n_cells))
    idx.train(base[:, :args.n_train].contiguous())
    for b0 in range(0, args.n, 250000):
        idx.add(base[:, b0:b0 + 250000].contiguous())
    idx.release_spare()
    idx.n_probe = args.n_probe

    ranks = (10, 100, 1000)
    top = idx.search(queries, k=max(ranks))[0]
    thresholds = {f"hits{r}": float(top[:, r - 1].median()) for r in ranks}
    thresholds["inf"] = float("inf")
    del top

    _, cells, npl = idx.probe(queries)
    cell_start, cell_size = idx._cell_start[cells].contiguous(), idx._cell_size[cells].contiguous()
    slots_hint = cells.shape[1] * idx.capacity // idx.n_cells
    scan_args = (idx._vectors(), queries, cell_start, cell_size, npl)
    scan_kw = dict(distance=idx.distance, slots_hint=slots_hint)

    legs = {"search_k100": lambda: idx.search(queries, k=args.k),
            "scan_k100_kernel": lambda: idx._flat_topk(*scan_args, args.k, **scan_kw)}
    for name, thr in thresholds.items():
        legs[f"range_{name}"] = lambda thr=thr: idx.range_search(queries, thr)
        legs[f"kernels_{name}"] = lambda thr=thr: idx._flat_range(*scan_args, thr, **scan_kw)
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    result = {"tool": "ivfflat_range_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "n_cells": args.n_cells, "n_probe": args.n_probe, "nq": args.nq, "k_yardstick": args.k,
              "steps": args.steps, "warmup": args.warmup, "index_bytes": int(idx._storage.numel()),
              "n_split": idx._flat_range.last_n_split, "thresholds": thresholds}
    for name, evs in events.items():
        result[name] = stats([a.elapsed_time(b) for a, b in evs], args.nq)
    yard, scan = result["search_k100"], result["scan_k100_kernel"]
    # the run's own spread of the yardstick, as a fraction of its median: what a ratio has to exceed 2 by to mean something
    result["yardstick_spread"] = round((yard["max_ms"] - yard["min_ms"]) / yard["median_ms"], 4)
    for name in thresholds:
        lims = out[f"range_{name}"][0]
        result[f"range_{name}"]["hits_per_query"] = round(float(lims[-1]) / args.nq, 2)
        result[f"range_{name}"]["over_search_k100"] = round(result[f"range_{name}"]["median_ms"] / yard["median_ms"], 4)
        result[f"kernels_{name}"]["over_scan_k100_kernel"] = round(
            result[f"kernels_{name}"]["median_ms"] / scan["median_ms"], 4)
        assert torch.equal(out[f"kernels_{name}"][0], lims)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
