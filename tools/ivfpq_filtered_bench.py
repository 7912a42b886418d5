#!/usr/bin/env python
"""What IVFPQIndex.search_filtered costs next to IVFPQIndex.search, and what it finds next to over-fetch-and-filter, at
the shape of bench.py's headline workload: the SIFT-like synthetic set, d = 128, m = 64, 1 024 cells, n_probe = 32,
1 M vectors, k = 100, 10 000 queries, in one process.

Filters are random id sets that pass a fraction `s` of the stored ids, s = 1, 0.5, 0.1, 0.01, 0.001.
Per step, interleaved (HIP-event timed after warm-up, median and spread over the steps; the filter's bit rows are built
before the timed window, their build is timed on its own):
  filtered_shared_s   search_filtered(queries, k, flt): one row shared by every query
  filtered_rows16_s   search_filtered(queries, k, flt16, rows): 16 rows of the same selectivity dealt over the queries
  search_k100         IVFPQIndex.search(k = 100) on the default route (the scan-layout kernels)
  search_k100_ref     the same with use_packed_layout = False: the reference-layout exact scan, the arithmetic and the
                      code layout the filtered scan uses -- the like-for-like yardstick
  search_k1024        IVFPQIndex.search(k = 1024): the over-fetch a caller without a filtered scan has to make
Reported: every leg's median / min / max, every filtered leg over both yardsticks, the yardsticks' own spread, and per
selectivity how many filtered neighbours a query has (of k) and how many of them over-fetch-and-filter finds in the
1 024 it fetched.  At s = 1 the filtered result is asserted equal to the reference-layout search, bit for bit.
Prints one JSON line and writes it to --out.

    python tools/ivfpq_filtered_bench.py [--n 1000000 --steps 10 --warmup 2 --out profiles/ivfpq_filtered_bench.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench import SiftLike, build_index  # noqa: E402
from tools.ivfflat_bench import stats, timed  # noqa: E402

SELECTIVITIES = (1.0, 0.5, 0.1, 0.01, 0.001)


def id_subset(ids, fraction, seed):
    if fraction >= 1.0:
        return ids
    g = torch.Generator(device=ids.device).manual_seed(seed)
    return ids[torch.rand(ids.numel(), device=ids.device, generator=g) < fraction].contiguous()


def found_by_overfetch(fetched_ids, allowed_ids, truth_ids):
    """per query: how many of its filtered neighbours (truth_ids, -1 padded) are among the fetched ids that pass the
    filter -> (mean neighbours a query has, mean of them found)"""
    allowed = torch.isin(fetched_ids, allowed_ids) & (fetched_ids >= 0)
    have = truth_ids >= 0
    hit = (truth_ids[:, :, None] == torch.where(allowed, fetched_ids, -2)[:, None, :]).any(2) & have
    return float(have.sum(1).float().mean()), float(hit.sum(1).float().mean())


def measure(idx, queries, args):
    nq, k, device = queries.shape[1], args.k, queries.device
    ids = idx._address2id[idx._address2id >= 0].contiguous()
    rows16 = (torch.arange(nq, device=device) % 16).to(torch.int32)
    shared, dealt, build_ms = {}, {}, {}
    for s in SELECTIVITIES:
        shared[s] = idx.id_filter(id_subset(ids, s, 100))
        dealt[s] = idx.id_filter([id_subset(ids, s, 200 + r) for r in range(16)])
        ev, _ = timed(lambda: shared[s].bits())          # one row from its ids: the id look-up and the bit kernel
        dealt[s].bits()
        torch.cuda.synchronize()
        build_ms[s] = round(ev[0].elapsed_time(ev[1]), 4)

    def search_ref(kk=k):
        idx.use_packed_layout = False
        try:
            return idx.search(queries, k=kk)
        finally:
            idx.use_packed_layout = True

    legs = {"search_k100": lambda: idx.search(queries, k=k),
            "search_k100_ref": search_ref,
            "search_k1024": lambda: idx.search(queries, k=1024)}
    for s in SELECTIVITIES:
        legs[f"filtered_shared_{s}"] = (lambda s=s: idx.search_filtered(queries, k, shared[s]))
        legs[f"filtered_rows16_{s}"] = (lambda s=s: idx.search_filtered(queries, k, dealt[s], rows16))
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    res = {"nq": nq, "k": k, "n_split": idx._ivfpq_filtered.last_n_split}
    for name, evs in events.items():
        res[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
    # every id allowed: the reference-layout search, bit for bit
    assert torch.equal(out["filtered_shared_1.0"][1], out["search_k100_ref"][1])
    assert torch.equal(out["filtered_shared_1.0"][0].view(torch.int32), out["search_k100_ref"][0].view(torch.int32))
    for yard in ("search_k100", "search_k100_ref"):
        res[f"{yard}_spread"] = round((res[yard]["max_ms"] - res[yard]["min_ms"]) / res[yard]["median_ms"], 4)
    res["selectivity"] = {}
    for s in SELECTIVITIES:
        row = {"filter_build_ms": build_ms[s], "allowed_ids": int(shared[s].ids[0].numel())}
        for form in ("shared", "rows16"):
            for yard in ("search_k100", "search_k100_ref"):
                row[f"{form}_over_{yard}"] = round(res[f"filtered_{form}_{s}"]["median_ms"] / res[yard]["median_ms"], 4)
        have, found = found_by_overfetch(out["search_k1024"][1], shared[s].ids[0], out[f"filtered_shared_{s}"][1])
        row["filtered_neighbours_per_query"] = round(have, 2)
        row["found_by_overfetch_1024"] = round(found, 2)
        res["selectivity"][str(s)] = row
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq_filtered_bench.json"))
    args = ap.parse_args()

    assert torch.cuda.is_available(), "ivfpq_filtered_bench measures on the GPU; there is nothing to report without one"
    device = torch.device("cuda:0")
    synth = SiftLike(args.d, device)
    base = synth.sample(args.n, seed=1)
    idx, _, _ = build_index(args, device, base, synth.sample(args.n_train, seed=2))
    idx.n_probe = args.n_probe
    nq = args.nq
    pick = torch.randperm(args.n, device=device, generator=torch.Generator(device=device).manual_seed(nq))[:nq]
    queries = (base[:, pick] + synth.noise * 0.25 * torch.randn(
        args.d, nq, device=device, generator=torch.Generator(device=device).manual_seed(nq + 1))).contiguous()
    result = {"tool": "ivfpq_filtered_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "m": args.m,
              "n": args.n, "n_cells": args.n_cells, "n_probe": args.n_probe, "steps": args.steps,
              "warmup": args.warmup, "index_bytes": int(idx._storage.numel()), **measure(idx, queries, args)}
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
