#!/usr/bin/env python
"""What FlatIndex.search_filtered / range_search_filtered cost at a SIFT1M-like shape, through the public API, against
the unfiltered fused search of the same run.

Every leg interleaved in one process (HIP-event timed, median and max - min over the steps):
  fused                 FlatIndex.search(k), use_fused_search = True: every slot walked on dense tiles
  filtered_<p>          search_filtered with a random <p> % of the ids allowed (100, 50, 10, 1, 0.1)
  filtered_two_rows     a batch whose queries alternate between the 10 % row and the 1 % row (one launch)
  overfetch_1           what a user does without it: search(k = 1024), cut by hand to the 1 % set -- with how many of
                        the k true filtered neighbours (search_filtered is the truth) it finds per query
  range_<p>             range_search_filtered at the density's own threshold of about --hits hits per query
Before timing, search_filtered with every id allowed is checked bit for bit against the fused search.
Prints one JSON line and writes it to --out.

    python tools/flat_filtered_bench.py [--n 1000000 --nq 1000 --k 100 --steps 10 --warmup 2]
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

from flat_bench import timed  # noqa: E402  (tools/ is the script's own directory)
from flat_range_bench import stats  # noqa: E402

DENSITIES = (100.0, 50.0, 10.0, 1.0, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--hits", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_filtered_bench.json"))
    args = ap.parse_args()

    from torchpq_amd.index import FlatIndex

    assert torch.cuda.is_available(), "flat_filtered_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    centers = torch.randn(args.d, 256, device="cuda", generator=gen) * 4
    pick = torch.randint(0, 256, (args.n,), device="cuda", generator=gen)
    base = (centers[:, pick] + torch.randn(args.d, args.n, device="cuda", generator=gen)).contiguous()
    flat = FlatIndex(args.d, initial_size=args.n)
    for b0 in range(0, args.n, 250000):
        flat.add(base[:, b0:b0 + 250000].contiguous())
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    del base, centers, pick
    flat.use_fused_search = True

    order = torch.randperm(args.n, device="cuda", generator=gen)       # a density's set: the first ids of one shuffle
    sets = {p: order[:max(1, int(args.n * p / 100))].contiguous() for p in DENSITIES}
    filters = {p: flat.id_filter(s) for p, s in sets.items()}
    two = flat.id_filter([sets[10.0], sets[1.0]])
    two_rows = (torch.arange(args.nq, device="cuda") % 2).to(torch.int32)
    for f in (*filters.values(), two):
        f.bits()                                                        # built once, outside the timed region
    name = lambda p: f"{p:g}".replace(".", "_")

    whole, every = flat.search(queries, k=args.k), flat.search_filtered(queries, args.k, filters[100.0])
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(whole, every)), \
        "search_filtered with every id allowed differs from the fused search"
    # thresholds of about --hits hits per query: the median value at that rank among the density's own neighbours
    k_thr = min(args.hits, 1024)
    thresholds = {p: float(flat.search_filtered(queries, k_thr, filters[p])[0][:, -1].clamp(min=-3e38).median())
                  for p in DENSITIES}
    member = torch.zeros(args.n, device="cuda", dtype=torch.bool)
    member[sets[1.0]] = True

    def overfetch():
        v, i = flat.search(queries, k=1024)
        keep = member[i.clamp(min=0)] & (i >= 0)
        rank = torch.cumsum(keep, 1)
        return v, torch.where(keep & (rank <= args.k), i, torch.full_like(i, -1))

    legs = {"fused": lambda: flat.search(queries, k=args.k)}
    for p in DENSITIES:
        legs["filtered_" + name(p)] = lambda p=p: flat.search_filtered(queries, args.k, filters[p])
    legs["filtered_two_rows"] = lambda: flat.search_filtered(queries, args.k, two, two_rows)
    legs["overfetch_1"] = overfetch
    for p in DENSITIES:
        legs["range_" + name(p)] = lambda p=p: flat.range_search_filtered(queries, thresholds[p], filters[p])
    events, out, parts = {leg: [] for leg in legs}, {}, {}
    for step in range(args.warmup + args.steps):
        for leg, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[leg] = timed(fn)
            if step >= args.warmup:
                events[leg].append(ev)
            parts[leg] = (flat._flat_range_filtered if leg.startswith("range_") else flat._flat_topk_filtered).last_n_parts
    torch.cuda.synchronize()
    result = {"tool": "flat_filtered_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "nq": args.nq, "k": args.k, "steps": args.steps, "warmup": args.warmup,
              "every_id_allowed_equals_fused_bitwise": True, "fused_n_parts": flat._flat_topk.last_n_parts, "legs": {}}
    fused_ms = None
    for leg, evs in events.items():
        row = stats([a.elapsed_time(b) for a, b in evs], args.nq)
        fused_ms = row["median_ms"] if leg == "fused" else fused_ms
        row["over_fused"] = round(row["median_ms"] / fused_ms, 4)
        if leg.startswith(("filtered_", "range_")):
            row["n_parts"] = parts[leg]
        if leg.startswith("range_"):
            row["hits_per_query"] = round(int(out[leg][0][-1]) / args.nq, 2)
        result["legs"][leg] = row
    truth = out["filtered_1"][1]
    found = (out["overfetch_1"][1][:, :, None] == truth[:, None, :]) & (truth[:, None, :] >= 0)
    result["legs"]["overfetch_1"]["true_neighbours_found_of_k"] = round(float(found.any(1).sum(1).float().mean()), 2)
    cheaper = [p for p in DENSITIES if result["legs"]["filtered_" + name(p)]["over_fused"] < 1.0]
    result["every_id_allowed_over_fused"] = result["legs"]["filtered_100"]["over_fused"]
    result["highest_measured_density_cheaper_than_fused_percent"] = max(cheaper) if cheaper else None
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
