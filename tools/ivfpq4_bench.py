#!/usr/bin/env python
"""What IVFPQ4Index.search costs next to IVFPQIndex.search, at the bench shape, through the public API.

Four indexes over the same vectors and the same coarse codebook, per step interleaved in one process (HIP-event timed,
median and spread over the steps):
  (a) IVFPQ4Index, m = --m      4-bit codes, m / 2 bytes per vector, no derived copy
  (b) IVFPQIndex,  m = --m      8-bit codes, twice the bytes, plus the scan-layout copy
  (c) IVFPQIndex,  m = --m / 2  8-bit codes, the same bytes as (a), plus the scan-layout copy
  (d) IVFPQ4Index, m = --m, pq_use_residual=True: (a)'s bytes, codes of x - centroid(cell), PQ trained on residuals,
      plus the cell-major copy of the coarse codebook (n_cells x d floats)
and (a) and (d) once more as their list scans alone (IVFPQ4TopkHip / IVFPQ4ResidualTopkHip on the coarse step's cells).
residual_over_plain_ms: (d) / (a) of the same run, for the search and for the scan kernel alone.
Reported per index: ms per batch (median, min, max), queries/s, the scanned code bytes per second -- bytes = sum over
(query, probe) of cell_size x code bytes (what the algorithm reads: every probed code once per query; the caches serve
most re-reads, so this is not an HBM rate), over the SEARCH time for the three indexes and over the kernel time for
the scan alone --, recall@k against FlatIndex.search, and the device memory of the codes plus any derived copy.
No figure is a target: (b) and (c) are the comparison points of (a), and (a) that of (d), measured in the same run.
Prints one JSON line and writes it to --out.

    python tools/ivfpq4_bench.py [--n 1000000 --nq 10000 --k 100 --steps 20 --warmup 3 --out profiles/ivfpq4_residual_bench.json]
(profiles/ivfpq4_bench.json is the record of the run before (d) existed.)
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

from tools.ivfflat_bench import clustered, recall, stats, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq4_residual_bench.json"))
    args = ap.parse_args()
    assert args.m % 16 == 0, "(a) needs m % 8 == 0, and (c) runs at m / 2"

    from torchpq_amd.index import FlatIndex, IVFPQ4Index, IVFPQIndex

    assert torch.cuda.is_available(), "ivfpq4_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    train = base[:, :args.n_train].contiguous()
    per_cell = max(64, 2 * args.n // args.n_cells)
    kw = dict(n_cells=args.n_cells, initial_size=per_cell)
    indexes = {"a_ivfpq4": IVFPQ4Index(args.d, n_subvectors=args.m, **kw),
               "b_ivfpq8": IVFPQIndex(args.d, n_subvectors=args.m, **kw),
               "c_ivfpq8_half_m": IVFPQIndex(args.d, n_subvectors=args.m // 2, **kw),
               "d_ivfpq4_residual": IVFPQ4Index(args.d, n_subvectors=args.m, pq_use_residual=True, **kw)}
    first, resid = indexes["a_ivfpq4"], indexes["d_ivfpq4_residual"]
    first.vq_codec.train(train)
    for idx in indexes.values():
        if idx is not first:
            idx.vq_codec.load_state_dict(first.vq_codec.state_dict())
        idx.pq_codec.train(idx._residual(train, idx.vq_codec.encode(train)) if idx is resid else train)
    flat = FlatIndex(args.d, initial_size=args.n)
    for b0 in range(0, args.n, 250000):
        chunk = base[:, b0:b0 + 250000].contiguous()
        for idx in indexes.values():
            idx.add(chunk)
        flat.add(chunk)
    for idx in indexes.values():
        idx.release_spare()
        idx.n_probe = args.n_probe

    sims, cells, npl = first.probe(queries)
    cell_start, cell_size = first._cell_start[cells].contiguous(), first._cell_size[cells].contiguous()
    probed = torch.arange(cells.shape[1], device=cells.device)[None, :] < npl[:, None]
    scanned_slots = int((cell_size * probed).sum().item())
    slots_hint = cells.shape[1] * first.capacity // first.n_cells

    legs = {name: (lambda idx=idx: idx.search(queries, k=args.k)) for name, idx in indexes.items()}
    legs["a_ivfpq4_scan_kernel"] = lambda: first._pq4_topk(
        first._storage, queries, first.pq_codec.codebook, cell_start, cell_size, npl, args.k,
        distance=first.distance, slots_hint=slots_hint)
    legs["d_ivfpq4_residual_scan_kernel"] = lambda: resid._pq4_topk(
        resid._storage, queries, resid.pq_codec.codebook, resid._cell_major_centroids(), cells,
        resid._cell_start[cells].contiguous(), resid._cell_size[cells].contiguous(), npl, args.k,
        distance=resid.distance, slots_hint=slots_hint)
    legs["flat_search"] = lambda: flat.search(queries, k=args.k)
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    result = {"tool": "ivfpq4_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "n_cells": args.n_cells, "n_probe": args.n_probe, "nq": args.nq, "k": args.k, "steps": args.steps,
              "warmup": args.warmup, "scanned_slots_per_query": round(scanned_slots / args.nq, 1),
              "n_split_ivfpq4": first._pq4_topk.last_n_split,
              "n_split_ivfpq4_residual": resid._pq4_topk.last_n_split}
    truth = out["flat_search"][1]
    for name in legs:
        leg = stats([a.elapsed_time(b) for a, b in events[name]], args.nq)
        idx = indexes.get(name, first if name.startswith("a_") else (resid if name.startswith("d_") else None))
        if idx is not None:
            code_bytes = int(idx.code_size)
            leg["m"] = int(idx.n_subvectors)
            leg["code_bytes_per_vector"] = code_bytes
            leg["scanned_code_gbytes_per_s"] = round(scanned_slots * code_bytes / (leg["median_ms"] * 1e-3) / 1e9, 1)
        if name in indexes:
            packed = getattr(idx, "_packed", None)
            leg["codes_bytes"] = int(idx._storage.numel())
            leg["derived_copy_bytes"] = int(packed.numel() * packed.element_size()) if packed is not None else 0
            if idx is resid:   # the cell-major coarse codebook the residual scan reads
                rows = resid._cell_major_centroids()
                leg["derived_copy_bytes"] = int(rows.numel() * rows.element_size())
            leg["device_bytes"] = leg["codes_bytes"] + leg["derived_copy_bytes"]
            leg["recall_at_k"] = recall(out[name][1], truth)
        result[name] = leg
    result["scan_ids_equal_search_ids"] = bool(torch.equal(
        first.get_id_by_address(out["a_ivfpq4_scan_kernel"][1]), out["a_ivfpq4"][1]))
    result["residual_scan_ids_equal_search_ids"] = bool(torch.equal(
        resid.get_id_by_address(out["d_ivfpq4_residual_scan_kernel"][1]), out["d_ivfpq4_residual"][1]))
    result["residual_over_plain_ms"] = {
        "search": round(result["d_ivfpq4_residual"]["median_ms"] / result["a_ivfpq4"]["median_ms"], 4),
        "scan_kernel": round(result["d_ivfpq4_residual_scan_kernel"]["median_ms"]
                             / result["a_ivfpq4_scan_kernel"]["median_ms"], 4)}
    by_time = sorted(indexes, key=lambda n: result[n]["median_ms"])
    by_recall = sorted(indexes, key=lambda n: -result[n]["recall_at_k"])
    result["fastest"], result["best_recall"] = by_time[0], by_recall[0]
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
