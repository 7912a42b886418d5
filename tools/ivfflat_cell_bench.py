#!/usr/bin/env python
"""IVFFlatIndex.search: the cell-major scan (use_cell_major, csrc/scan_flat_cells.hip) against the query-major scan, at
the shape of DESIGN 3.8, through the public API, both routes in one process.

Per step, interleaved (HIP-event timed, median / min / max over the steps), for every batch size of --batches:
  off                       IVFFlatIndex.search(k) with the switch off
  on p<P0> c<cap>           the same search with the switch on, for every first_probe of --first-probes and cand_cap of
                            --cand-caps
Per setting also: the candidates per query (mean, max) and the redone queries, whether the results equal the switch-off
results bit for bit, and the time of each of the five stages -- the library call alone, ended behind stage 1 ... 5
(tpq_ivf_flat_cells_stop_after), medians of the cumulative times differenced.
Prints one JSON line and writes it to --out.

    python tools/ivfflat_cell_bench.py [--n 1000000 --k 100 --steps 10 --warmup 2 --out profiles/ivfflat_cell_bench.json]
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

from tools.ivfflat_bench import clustered, timed  # noqa: E402


def stats(ms):
    ms = np.asarray(ms)
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(float(ms.min()), 4),
            "max_ms": round(float(ms.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[1024, 4096, 10000])
    ap.add_argument("--first-probes", type=int, nargs="+", default=[1, 2, 4])
    ap.add_argument("--cand-caps", type=int, nargs="+", default=[512, 1024, 2048])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_cell_bench.json"))
    args = ap.parse_args()

    from torchpq_amd._lib import load, ptr
    from torchpq_amd.index import IVFFlatIndex
    from torchpq_amd.kernels._common import alloc_pair, call, metric_code

    assert torch.cuda.is_available(), "ivfflat_cell_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    nq_max = max(args.batches)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:nq_max]]
               + 0.3 * torch.randn(args.d, nq_max, device="cuda", generator=gen)).contiguous()
    idx = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=max(64, 2 * args.n // args.n_cells))
    idx.train(base[:, :args.n_train].contiguous())
    for b0 in range(0, args.n, 250000):
        idx.add(base[:, b0:b0 + 250000].contiguous())
    idx.release_spare()
    idx.n_probe = args.n_probe
    idx.cell_major_min_batch = 1
    op = idx._flat_cells
    op.keep_workspace = True
    settings = [(p0, cap) for p0 in args.first_probes for cap in args.cand_caps]

    def search(x, on, p0=None, cap=None):
        idx.use_cell_major = on
        if on:
            op.first_probe, op.cand_cap = p0, cap
        return idx.search(x, k=args.k, return_address=True)

    def stage_call(x, cells, cs, sz, npl, p0, cap):
        """the library call alone on the coarse step's cells: no read-back, no redo"""
        nq = x.shape[1]
        vals, addr = alloc_pair(nq, args.k, x.device)
        nb = load().tpq_ivf_flat_cells_workspace_bytes(nq, cells.shape[1], idx.n_cells, args.k, cap, p0)
        ws = torch.empty(nb, device=x.device, dtype=torch.uint8)
        vec = idx._vectors()
        return lambda: call("tpq_ivf_flat_cells_topk", x.device, ptr(vec), ptr(x), None, ptr(cells), ptr(cs), ptr(sz),
                            ptr(npl), ptr(vals), ptr(addr), vec.shape[1], idx.n_cells, args.d, nq, cells.shape[1], args.k,
                            metric_code(idx.distance), p0, cap, ptr(ws), nb)

    result = {"tool": "ivfflat_cell_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "n_cells": args.n_cells, "n_probe": args.n_probe, "k": args.k, "steps": args.steps,
              "warmup": args.warmup, "batches": {}}
    for nq in args.batches:
        x = queries[:, :nq].contiguous()
        legs = {"off": lambda: search(x, False)}
        for p0, cap in settings:
            legs[f"on p{p0} c{cap}"] = lambda p0=p0, cap=cap: search(x, True, p0, cap)
        _, cells, npl = idx.probe(x)
        cells = cells.contiguous()
        cs, sz = idx._cell_start[cells].contiguous(), idx._cell_size[cells].contiguous()
        stage_legs = {(p0, cap): stage_call(x, cells, cs, sz, npl, p0, cap) for p0, cap in settings}
        events = {name: [] for name in legs}
        stage_events = {(key, stop): [] for key in stage_legs for stop in range(1, 6)}
        out, info = {}, {}
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():          # interleaved: every leg sees the same clocks
                ev, out[name] = timed(fn)
                if step >= args.warmup:
                    events[name].append(ev)
                if name != "off" and name not in info:
                    A = (nq * 4 + 255) // 256 * 256
                    cnt = op.last_workspace[256 + 3 * A:256 + 3 * A + 4 * nq].view(torch.int32)
                    info[name] = {"candidates_mean": round(float(cnt.float().mean()), 1), "candidates_max": int(cnt.max()),
                                  "redone": op.last_redone}
            for key, fn in stage_legs.items():
                for stop in range(1, 6):
                    before = load().tpq_ivf_flat_cells_stop_after(stop % 5)
                    try:
                        ev, _ = timed(fn)
                    finally:
                        load().tpq_ivf_flat_cells_stop_after(before)
                    if step >= args.warmup:
                        stage_events[(key, stop)].append(ev)
        torch.cuda.synchronize()
        rec = {"off": stats([a.elapsed_time(b) for a, b in events["off"]])}
        for p0, cap in settings:
            name = f"on p{p0} c{cap}"
            r = stats([a.elapsed_time(b) for a, b in events[name]])
            r.update(info[name])
            r["equal_to_off"] = all(bool(torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g, w.view(torch.int32)
                                                     if w.dtype == torch.float32 else w))
                                    for g, w in zip(out[name], out["off"]))
            r["ratio_off_over_on"] = round(rec["off"]["median_ms"] / r["median_ms"], 3)
            cum = [float(np.median([a.elapsed_time(b) for a, b in stage_events[((p0, cap), s)]])) for s in range(1, 6)]
            r["stage_ms"] = {f"stage{s + 1}": round(cum[s] - (cum[s - 1] if s else 0.0), 4) for s in range(5)}
            rec[name] = r
        result["batches"][str(nq)] = rec
        del out
    idx.use_cell_major = False
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
