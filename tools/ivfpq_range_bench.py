#!/usr/bin/env python
"""What IVFPQIndex.range_search costs next to IVFPQIndex.search, at the shape of bench.py's headline workload: the
SIFT-like synthetic set, d = 128, m = 64, 1 024 cells, n_probe = 32, 1 M vectors; 10 000 queries and 100 queries.

Thresholds: per query, the 100th value of search(k = 100) -- about 100 hits per query (more where values tie).
Per step, interleaved in one process (HIP-event timed after warm-up, median and spread over the steps):
  range_search       IVFPQIndex.range_search(queries, thresholds): coarse step, count pass, prefix sum, host sync, fill
                     pass, address -> id
  search_k100        IVFPQIndex.search(k = 100) on the default route (the scan-layout kernels)
  search_k100_ref    the same with use_packed_layout = False: the reference-layout exact scan, the arithmetic and the
                     code layout the range passes use -- the like-for-like yardstick
  count_kernel / fill_kernel    the two passes alone (tpq_ivfpq_range_count / _fill) on the coarse step's cells
range_search ends with a host sync (the hit count sizes the outputs), so its event pair spans the device work of the
call; the other legs are asynchronous and their pairs span the device work likewise.
Reported per batch size: every leg's median / min / max, range_search over both yardsticks, the yardstick's own
spread, hits per query, the workgroups per query of the range passes, and the peak temporary memory of one
range_search call (torch's allocator: peak minus what was allocated before the call).
Prints one JSON line and writes it to --out.

    python tools/ivfpq_range_bench.py [--n 1000000 --steps 20 --warmup 3 --out profiles/ivfpq_range_bench.json]
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


def passes_alone(idx, queries, thr):
    """(count, fill, hits): the two launches on the coarse step's cells, as IVFPQRangeHip makes them (table built in the
    workgroup), each callable on its own; the offsets are formed once, outside the timed calls"""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    _, cells, npl = idx.probe(queries)
    nq, n_probe = cells.shape
    cs, sz = idx._cell_start[cells].contiguous(), idx._cell_size[cells].contiguous()
    op = idx._ivfpq_range
    n_split = op._n_split(nq, queries.device, n_probe * idx.capacity // idx.n_cells)
    n_seg = lib.tpq_ivfpq_range_segments(nq, n_split)
    codes, cb = idx._scan_codes(), idx.pq_codec.codebook.contiguous()
    is_empty = idx._is_empty if idx._has_holes else None
    inputs = (ptr(codes), None, ptr(queries), ptr(cb), idx.d_subvector, 0, ptr(is_empty), ptr(cs), ptr(sz), ptr(npl),
              ptr(thr))
    shape = (codes.shape[1], nq, n_probe, idx.n_subvectors, n_split)
    counts = torch.empty(n_seg, device=queries.device, dtype=torch.int32)
    keep = [cells, npl, cs, sz, cb, counts]

    def count():
        check(lib.tpq_ivfpq_range_count(*inputs, ptr(counts), *shape, stream_ptr(queries.device)), "count")

    count()
    offsets = torch.zeros(n_seg + 1, device=queries.device, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[-1])
    vals = torch.empty(total, device=queries.device, dtype=torch.float32)
    addr = torch.empty(total, device=queries.device, dtype=torch.int64)
    keep += [offsets, vals, addr]

    def fill():
        check(lib.tpq_ivfpq_range_fill(*inputs, ptr(offsets), ptr(vals), ptr(addr), *shape,
                                       stream_ptr(queries.device)), "fill")
        return keep

    return count, fill, total, n_split


def measure(idx, queries, args):
    nq = queries.shape[1]
    thr = idx.search(queries, k=args.k)[0][:, args.k - 1].contiguous()
    thr = torch.where(torch.isfinite(thr), thr, torch.full_like(thr, -3.0e38))
    count, fill, total, n_split = passes_alone(idx, queries, thr)

    def search_ref():
        idx.use_packed_layout = False
        try:
            return idx.search(queries, k=args.k)
        finally:
            idx.use_packed_layout = True

    legs = {"range_search": lambda: idx.range_search(queries, thr),
            "search_k100": lambda: idx.search(queries, k=args.k),
            "search_k100_ref": search_ref,
            "count_kernel": count,
            "fill_kernel": fill}
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    res = {"nq": nq, "n_split": n_split}
    for name, evs in events.items():
        res[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
    lims = out["range_search"][0]
    assert int(lims[-1]) == total                      # the passes alone found what range_search found
    assert torch.equal(out["search_k100"][0], out["search_k100_ref"][0])     # both routes: the same bits
    res["hits_per_query"] = round(total / nq, 2)
    for yard in ("search_k100", "search_k100_ref"):
        res[f"range_over_{yard}"] = round(res["range_search"]["median_ms"] / res[yard]["median_ms"], 4)
        res[f"{yard}_spread"] = round((res[yard]["max_ms"] - res[yard]["min_ms"]) / res[yard]["median_ms"], 4)
    res["passes_over_search_k100_ref"] = round(
        (res["count_kernel"]["median_ms"] + res["fill_kernel"]["median_ms"]) / res["search_k100_ref"]["median_ms"], 4)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    idx.range_search(queries, thr)
    torch.cuda.synchronize()
    res["range_peak_temporary_bytes"] = int(torch.cuda.max_memory_allocated() - before)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--nq", type=int, nargs="+", default=[10000, 100])
    ap.add_argument("--k", type=int, default=100, help="k of the yardstick search; the thresholds are its k-th values")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfpq_range_bench.json"))
    args = ap.parse_args()

    assert torch.cuda.is_available(), "ivfpq_range_bench measures on the GPU; there is nothing to report without one"
    device = torch.device("cuda:0")
    synth = SiftLike(args.d, device)
    base = synth.sample(args.n, seed=1)
    idx, _, _ = build_index(args, device, base, synth.sample(args.n_train, seed=2))
    idx.n_probe = args.n_probe
    result = {"tool": "ivfpq_range_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "m": args.m,
              "n": args.n, "n_cells": args.n_cells, "n_probe": args.n_probe, "k_yardstick": args.k,
              "steps": args.steps, "warmup": args.warmup, "index_bytes": int(idx._storage.numel()), "batches": []}
    for nq in args.nq:
        pick = torch.randperm(args.n, device=device, generator=torch.Generator(device=device).manual_seed(nq))[:nq]
        queries = (base[:, pick] + synth.noise * 0.25 * torch.randn(
            args.d, nq, device=device, generator=torch.Generator(device=device).manual_seed(nq + 1))).contiguous()
        result["batches"].append(measure(idx, queries, args))
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
