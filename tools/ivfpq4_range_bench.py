#!/usr/bin/env python
"""What IVFPQ4Index.range_search and range_search_filtered cost next to IVFPQ4Index.search, at the shape of
tools/ivfpq4_bench.py: 1 M clustered vectors, d = 128, m = 64, 1 024 cells, n_probe = 32, 10 000 queries.

Thresholds: per query, the k-th value of search(k = 100) of the same index -- about 100 hits per query (more where
values tie).  Per index, per step, interleaved in one process (HIP-event timed after warm-up, median and spread over
the steps):
  search_k100             IVFPQ4Index.search(k = 100): the yardstick, the same index in the same process
  range_search            IVFPQ4Index.range_search(queries, thresholds): coarse step, count pass, prefix sum, host sync,
                          fill pass, address -> id
  range_filtered_<pct>    IVFPQ4Index.range_search_filtered under a filter that allows <pct> % of the ids (100, 10, 1,
                          0.1; one row, every query), the same thresholds
range_search ends with a host sync (the hit count sizes the outputs), so its event pair spans the device work of the
call; search is asynchronous and its pair spans the device work likewise.
Three indexes: plain codes and residual codes over --n-cells cells, and residual codes once more over --n-short-cells
short cells (one workgroup per (query, probe) then builds a table for a cell of a tile or so: where the table build would
show between workgroups, it shows here).  Reported per index: every leg's median / min / max, every range leg over the
index's own search_k100, the yardstick's spread, hits per query, the workgroups per query of the plain passes.
No figure is a target.  Prints one JSON line and writes it to --out.  Reads nothing outside the repository.

    python tools/ivfpq4_range_bench.py [--n 1000000 --steps 10 --warmup 2 --out profiles/ivfpq4_range_bench.json]
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

PERCENTS = (100.0, 10.0, 1.0, 0.1)


def build(args, base, train, n_cells, residual, coarse=None):
    """an IVFPQ4Index over `base`; `coarse`: an index whose trained coarse codebook is taken over"""
    from torchpq_amd.index import IVFPQ4Index
    idx = IVFPQ4Index(args.d, n_subvectors=args.m, n_cells=n_cells, initial_size=max(64, 2 * args.n // n_cells),
                      pq_use_residual=residual)
    if coarse is None:
        idx.vq_codec.train(train)
    else:
        idx.vq_codec.load_state_dict(coarse.vq_codec.state_dict())
    idx.pq_codec.train(idx._residual(train, idx.vq_codec.encode(train)) if residual else train)
    for b0 in range(0, args.n, 250000):
        idx.add(base[:, b0:b0 + 250000].contiguous())
    idx.release_spare()
    idx.n_probe = args.n_probe
    return idx


def measure(idx, queries, args, gen):
    nq = queries.shape[1]
    thr = idx.search(queries, k=args.k)[0][:, args.k - 1].contiguous()
    thr = torch.where(torch.isfinite(thr), thr, torch.full_like(thr, -3.0e38))
    ids = idx._address2id[idx._address2id >= 0]
    legs = {"search_k100": lambda: idx.search(queries, k=args.k),
            "range_search": lambda: idx.range_search(queries, thr)}
    for pct in PERCENTS:
        n_allowed = max(1, int(round(ids.numel() * pct / 100.0)))
        pick = ids if pct == 100.0 else ids[torch.randperm(ids.numel(), device=ids.device, generator=gen)[:n_allowed]]
        flt = idx.id_filter(pick.contiguous())
        legs["range_filtered_%g" % pct] = lambda flt=flt: idx.range_search_filtered(queries, thr, flt)
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    res = {"n_cells": int(idx.n_cells), "pq_use_residual": bool(idx.pq_use_residual), "nq": nq,
           "n_split_range": idx._pq4_range.last_n_split, "n_split_search": idx._pq4_topk.last_n_split}
    for name, evs in events.items():
        res[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
    yard = res["search_k100"]
    res["search_k100_spread"] = round((yard["max_ms"] - yard["min_ms"]) / yard["median_ms"], 4)
    for name in legs:
        if name != "search_k100":
            res[name]["hits_per_query"] = round(int(out[name][0][-1]) / nq, 2)
            res[name]["over_search_k100"] = round(res[name]["median_ms"] / yard["median_ms"], 4)
    # the all-ids filter finds what the unfiltered search finds
    assert torch.equal(out["range_filtered_100"][0], out["range_search"][0])
    assert torch.equal(out["range_filtered_100"][2], out["range_search"][2])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-short-cells", type=int, default=16384, help="0: skip the short-cell residual index")
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100, help="k of the yardstick search; the thresholds are its k-th values")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq4_range_bench.json"))
    args = ap.parse_args()

    assert torch.cuda.is_available(), "ivfpq4_range_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    train = base[:, :args.n_train].contiguous()
    result = {"tool": "ivfpq4_range_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "m": args.m,
              "n": args.n, "n_probe": args.n_probe, "nq": args.nq, "k_yardstick": args.k, "steps": args.steps,
              "warmup": args.warmup, "indexes": {}}
    say = lambda what: print("ivfpq4_range_bench: " + what, file=sys.stderr, flush=True)
    say("plain codes, %d cells" % args.n_cells)
    plain = build(args, base, train, args.n_cells, False)
    result["indexes"]["plain"] = measure(plain, queries, args, gen)
    say("residual codes, %d cells" % args.n_cells)
    resid = build(args, base, train, args.n_cells, True, coarse=plain)
    del plain
    result["indexes"]["residual"] = measure(resid, queries, args, gen)
    del resid
    if args.n_short_cells:
        say("residual codes, %d cells" % args.n_short_cells)
        short = build(args, base, train, args.n_short_cells, True)
        result["indexes"]["residual_short_cells"] = measure(short, queries, args, gen)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
