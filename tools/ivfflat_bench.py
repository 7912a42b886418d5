#!/usr/bin/env python
"""What IVFFlatIndex.search costs, at a SIFT1M-like shape, through the public API.

Per step, interleaved in one process (HIP-event timed, median and spread over the steps):
  (a) IVFFlatIndex.search(k)            coarse step + list scan + address -> id
  (b) the list scan alone (IVFFlatTopkHip) on the coarse step's cells
  (c) FlatIndex.search(k)               exact search over everything, the recall ground truth
  (d) IVFPQIndex.search(k), m = --m     the compressed index on the same vectors and the same coarse codebook
Reported: queries/s of each leg; for (b) the scanned bytes/s, bytes = sum over (query, probe) of cell_size x 4 d (what
the algorithm reads: every probed vector once per query; the caches serve most re-reads, so this rate is not an HBM
rate) and its fraction of the box's measured stream peak (bench.py's own sweep); recall@k of (a) and (d) against (c).
Prints one JSON line and writes it to --out.

    python tools/ivfflat_bench.py [--n 1000000 --nq 10000 --k 100 --steps 20 --warmup 3 --out profiles/ivfflat_bench.json]
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


def clustered(d, n, n_centers, gen):
    centers = torch.randn(d, n_centers, device="cuda", generator=gen) * 4
    pick = torch.randint(0, n_centers, (n,), device="cuda", generator=gen)
    return (centers[:, pick] + torch.randn(d, n, device="cuda", generator=gen)).contiguous()


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


def recall(ids, truth):
    """mean fraction of the true k nearest that were returned"""
    hit = (ids[:, :, None] == truth[:, None, :]).any(1)
    return round(float(hit.float().mean()), 6)


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
    ap.add_argument("--stream-gib", type=int, default=8, help="buffer of the stream-peak sweep (0 = skip it)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_bench.json"))
    args = ap.parse_args()

    from torchpq_amd.index import FlatIndex, IVFFlatIndex, IVFPQIndex

    assert torch.cuda.is_available(), "ivfflat_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    per_cell = max(64, 2 * args.n // args.n_cells)
    idx = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=per_cell)
    idx.train(base[:, :args.n_train].contiguous())
    pq = IVFPQIndex(args.d, n_subvectors=args.m, n_cells=args.n_cells, initial_size=per_cell)
    pq.vq_codec.load_state_dict(idx.vq_codec.state_dict())
    pq.pq_codec.train(base[:, :args.n_train].contiguous())
    flat = FlatIndex(args.d, initial_size=args.n)
    for b0 in range(0, args.n, 250000):
        chunk = base[:, b0:b0 + 250000].contiguous()
        idx.add(chunk)
        pq.add(chunk)
        flat.add(chunk)
    idx.release_spare()
    pq.release_spare()
    idx.n_probe = pq.n_probe = args.n_probe

    sims, cells, npl = idx.probe(queries)
    cell_start, cell_size = idx._cell_start[cells].contiguous(), idx._cell_size[cells].contiguous()
    probed = torch.arange(cells.shape[1], device=cells.device)[None, :] < npl[:, None]
    scanned_slots = int((cell_size * probed).sum().item())
    scanned_bytes = scanned_slots * 4 * args.d
    slots_hint = cells.shape[1] * idx.capacity // idx.n_cells

    legs = {
        "a_ivfflat_search": lambda: idx.search(queries, k=args.k),
        "b_ivfflat_scan_kernel": lambda: idx._flat_topk(idx._vectors(), queries, cell_start, cell_size, npl, args.k,
                                                        distance=idx.distance, slots_hint=slots_hint),
        "c_flat_search": lambda: flat.search(queries, k=args.k),
        "d_ivfpq_search": lambda: pq.search(queries, k=args.k),
    }
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    result = {"tool": "ivfflat_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "n_cells": args.n_cells, "n_probe": args.n_probe, "m_ivfpq": args.m, "nq": args.nq, "k": args.k,
              "steps": args.steps, "warmup": args.warmup, "index_bytes": int(idx._storage.numel()),
              "n_split": idx._flat_topk.last_n_split}
    for name, evs in events.items():
        result[name] = stats([a.elapsed_time(b) for a, b in evs], args.nq)
    scan_s = result["b_ivfflat_scan_kernel"]["median_ms"] * 1e-3
    result["scanned_slots_per_query"] = round(scanned_slots / args.nq, 1)
    result["scanned_bytes"] = scanned_bytes
    result["scanned_gbytes_per_s"] = round(scanned_bytes / scan_s / 1e9, 1)
    truth = out["c_flat_search"][1]
    result["recall_at_k_ivfflat"] = recall(out["a_ivfflat_search"][1], truth)
    result["recall_at_k_ivfpq"] = recall(out["d_ivfpq_search"][1], truth)
    result["scan_ids_equal_search_ids"] = bool(torch.equal(idx.get_id_by_address(out["b_ivfflat_scan_kernel"][1]),
                                                           out["a_ivfflat_search"][1]))
    del out
    torch.cuda.empty_cache()
    if args.stream_gib:
        from bench import stream_peak_gbps
        peak = stream_peak_gbps("cuda:0", gib=args.stream_gib)
        result["stream_peak_gbytes_per_s"] = round(peak, 1)
        # (re-reads of a cell by later queries are served by L2 / the Infinity Cache: the fraction may exceed 1)
        result["scanned_rate_over_stream_peak"] = round(result["scanned_gbytes_per_s"] / peak, 4)
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
