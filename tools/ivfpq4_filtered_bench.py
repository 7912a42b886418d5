#!/usr/bin/env python
"""What IVFPQ4Index.search_filtered costs next to IVFPQ4Index.search, and what it finds next to over-fetch-and-filter,
at the shape of tools/ivfpq4_bench.py: 1 M x 128 clustered vectors, m = 64, 1 024 cells, n_probe = 32, k = 100,
10 000 queries, in one process -- with plain codes, with residual codes, and with residual codes over 16 384 cells
(short cells: the per-probe tables weigh most there).

Filters are random id sets that pass a fraction `s` of the stored ids, s = 1, 0.5, 0.1, 0.01, 0.001.
Per index and step, interleaved (HIP-event timed after warm-up, median and spread over the steps; the filter's bit rows
are built before the timed window):
  search_k100         IVFPQ4Index.search(k = 100): the yardstick
  filtered_shared_s   search_filtered(queries, k, flt): one row shared by every query
  filtered_rows16_s   search_filtered(queries, k, flt16, rows): 16 rows of the same selectivity dealt over the queries
  search_k1024        IVFPQ4Index.search(k = 1024): the over-fetch a caller without a filtered scan has to make
Reported per index: every leg's median / min / max, every filtered leg over the yardstick, the yardstick's own spread,
and per selectivity how many filtered neighbours a query has (of k) and how many of them over-fetch-and-filter finds in
the 1 024 it fetched.  At s = 1 the filtered result is asserted equal to search, bit for bit.
(`measure` and `run` take extra legs: tools/experiments/pq4_filtered_ab.py adds the A/B legs of a kernel variant to the
same interleaved loop and records them under "ab" in the same profile.)
Prints one JSON line and writes it to --out.

    python tools/ivfpq4_filtered_bench.py [--n 1000000 --steps 10 --warmup 2 --out profiles/ivfpq4_filtered_bench.json]
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
from tools.ivfpq_filtered_bench import SELECTIVITIES, found_by_overfetch, id_subset  # noqa: E402

INDEXES = ("plain_1024", "residual_1024", "residual_16384")


def measure(idx, queries, args, extra=None):
    """one index; `extra`: an object with legs(idx, queries, k, shared) -> {name: fn}, more legs for the interleaved
    loop, and finish(res, out), which gets every leg's statistics and last result"""
    nq, k, device = queries.shape[1], args.k, queries.device
    ids = idx._address2id[idx._address2id >= 0].contiguous()
    rows16 = (torch.arange(nq, device=device) % 16).to(torch.int32)
    shared, dealt = {}, {}
    for s in SELECTIVITIES:
        shared[s] = idx.id_filter(id_subset(ids, s, 100))
        dealt[s] = idx.id_filter([id_subset(ids, s, 200 + r) for r in range(16)])
        shared[s].bits()
        dealt[s].bits()
    torch.cuda.synchronize()
    legs = {"search_k100": lambda: idx.search(queries, k=k),
            "search_k1024": lambda: idx.search(queries, k=1024)}
    for s in SELECTIVITIES:
        legs[f"filtered_shared_{s}"] = (lambda s=s: idx.search_filtered(queries, k, shared[s]))
        legs[f"filtered_rows16_{s}"] = (lambda s=s: idx.search_filtered(queries, k, dealt[s], rows16))
    if extra is not None:
        legs.update(extra.legs(idx, queries, k, shared))
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    res = {"n_cells": idx.n_cells, "pq_use_residual": idx.pq_use_residual,
           "n_split": idx._pq4_filtered.last_n_split}
    for name, evs in events.items():
        res[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
    # every id allowed: search, bit for bit
    assert torch.equal(out["filtered_shared_1.0"][1], out["search_k100"][1])
    assert torch.equal(out["filtered_shared_1.0"][0].view(torch.int32), out["search_k100"][0].view(torch.int32))
    if extra is not None:
        extra.finish(res, out)
    yard = res["search_k100"]
    res["search_k100_spread"] = round((yard["max_ms"] - yard["min_ms"]) / yard["median_ms"], 4)
    res["selectivity"] = {}
    for s in SELECTIVITIES:
        row = {"allowed_ids": int(shared[s].ids[0].numel())}
        for form in ("shared", "rows16"):
            row[f"{form}_over_search_k100"] = round(res[f"filtered_{form}_{s}"]["median_ms"] / yard["median_ms"], 4)
        have, found = found_by_overfetch(out["search_k1024"][1], shared[s].ids[0], out[f"filtered_shared_{s}"][1])
        row["filtered_neighbours_per_query"] = round(have, 2)
        row["found_by_overfetch_1024"] = round(found, 2)
        res["selectivity"][str(s)] = row
    return res


def parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default=",".join(INDEXES), help="comma-separated subset of " + ", ".join(INDEXES))
    ap.add_argument("--label", default="product", help="the library variant measured (recorded in the result)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq4_filtered_bench.json"))
    return ap


def run(args, extra=None):
    """build every index of --only and measure it -> the result record"""
    only = [name for name in args.only.split(",") if name]
    assert only and set(only) <= set(INDEXES), only

    from torchpq_amd import _lib
    from torchpq_amd.index import IVFPQ4Index

    assert torch.cuda.is_available(), "ivfpq4_filtered_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    train = base[:, :args.n_train].contiguous()
    result = {"tool": "ivfpq4_filtered_bench", "label": args.label, "library": os.path.basename(_lib.LIB_PATH),
              "device": torch.cuda.get_device_name(0), "d": args.d, "m": args.m, "n": args.n, "n_probe": args.n_probe,
              "nq": args.nq, "k": args.k, "steps": args.steps, "warmup": args.warmup}
    for name in only:
        kind, n_cells = name.split("_")
        n_cells = int(n_cells)
        idx = IVFPQ4Index(args.d, n_subvectors=args.m, n_cells=n_cells, initial_size=max(64, 2 * args.n // n_cells),
                          pq_use_residual=(kind == "residual"))
        idx.train(train)
        for b0 in range(0, args.n, 250000):
            idx.add(base[:, b0:b0 + 250000].contiguous())
        idx.release_spare()
        idx.n_probe = args.n_probe
        result[name] = measure(idx, queries, args, extra if kind == "residual" else None)
        result[name]["index_bytes"] = int(idx._storage.numel())
        del idx
        torch.cuda.empty_cache()
    return result


def main():
    args = parser().parse_args()
    line = json.dumps(run(args))
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
