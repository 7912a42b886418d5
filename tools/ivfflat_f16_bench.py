#!/usr/bin/env python
"""IVFFlat16Index.search (fp16-stored lists, csrc/scan_flat_f16.hip) against IVFFlatIndex.search on the same data and
the same coarse codebook, at the shape of DESIGN 3.8, through the public API, all legs in one process.

Per step, interleaved (HIP-event timed, median / min / max over the steps), for every batch size of --batches:
  fp32 query-major          IVFFlatIndex.search(k), use_cell_major off
  fp32 cell-major           IVFFlatIndex.search(k), use_cell_major on
  fp16 query-major          IVFFlat16Index.search(k), use_cell_major off
  fp16 cell-major           IVFFlat16Index.search(k), use_cell_major on (csrc/scan_flat_f16_cells.hip)
and, on the coarse step's cells, the two list scans alone (IVFFlatTopkHip, IVFFlat16TopkHip) with the bytes they scan:
sum over (query, probe) of cell_size x code_size -- what the algorithm reads, served mostly by the caches, so not an HBM
rate.  Also: whether each cell-major route returns its query-major route's ids, the candidates per query of both
cell-major routes (the `cnt` words of a kept workspace from one more, untimed search: the fp16 route's band is wider,
and this is where it shows), the device bytes of both storages and the mean overlap of the fp16 index's top-k ids with the fp32 index's.
Prints one JSON line and writes it to --out.

    python tools/ivfflat_f16_bench.py [--n 1000000 --k 100 --steps 10 --warmup 3 --out profiles/ivfflat_f16_bench.json]
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

from tools.ivfflat_bench import clustered, recall, timed  # noqa: E402
from tools.ivfflat_cell_bench import stats  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--batches", type=int, nargs="+", default=[10000, 1024, 64])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_f16_bench.json"))
    args = ap.parse_args()

    from torchpq_amd.index import IVFFlat16Index, IVFFlatIndex

    assert torch.cuda.is_available(), "ivfflat_f16_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    nq_max = max(args.batches)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:nq_max]]
               + 0.3 * torch.randn(args.d, nq_max, device="cuda", generator=gen)).contiguous()
    per_cell = max(64, 2 * args.n // args.n_cells)
    f32 = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=per_cell)
    f32.train(base[:, :args.n_train].contiguous())
    f16 = IVFFlat16Index(args.d, n_cells=args.n_cells, initial_size=per_cell)
    f16.vq_codec.load_state_dict(f32.vq_codec.state_dict())
    for b0 in range(0, args.n, 250000):
        chunk = base[:, b0:b0 + 250000].contiguous()
        f32.add(chunk)
        f16.add(chunk)
    for idx in (f32, f16):
        idx.release_spare()
        idx.n_probe = args.n_probe
        idx.cell_major_min_batch = 1

    def search(idx, x, cell_major):
        idx.use_cell_major = cell_major
        return idx.search(x, k=args.k)

    def candidates(idx, x):
        """mean and maximum candidates per query of the index's cell-major route: the i32 [nq] `cnt` region of the
        workspace (behind the control words, the flags, the thresholds and |q|^2: include/torchpq_amd.h)"""
        idx._flat_cells.keep_workspace = True
        search(idx, x, True)
        nq = x.shape[1]
        at = 256 + 3 * ((4 * nq + 255) // 256 * 256)
        cnt = idx._flat_cells.last_workspace[at:at + 4 * nq].view(torch.int32).double()
        idx._flat_cells.keep_workspace, idx._flat_cells.last_workspace = False, None
        return {"mean": round(cnt.mean().item(), 1), "max": int(cnt.max().item()),
                "redone": int(idx._flat_cells.last_redone), "cand_cap": idx._flat_cells.cand_cap}

    def scan_leg(idx, x):
        """the list scan alone on the index's own coarse cells -> (call, scanned bytes)"""
        _, cells, npl = idx.probe(x)
        cs, sz = idx._cell_start[cells].contiguous(), idx._cell_size[cells].contiguous()
        probed = torch.arange(cells.shape[1], device=cells.device)[None, :] < npl[:, None]
        scanned = int((sz * probed).sum().item()) * idx.code_size
        hint = cells.shape[1] * idx.capacity // idx.n_cells
        return (lambda: idx._flat_topk(idx._vectors(), x, cs, sz, npl, args.k, distance=idx.distance, slots_hint=hint),
                scanned)

    result = {"tool": "ivfflat_f16_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "n_cells": args.n_cells, "n_probe": args.n_probe, "k": args.k, "steps": args.steps,
              "warmup": args.warmup, "storage_bytes_fp32": int(f32._storage.numel()),
              "storage_bytes_fp16": int(f16._storage.numel()), "batches": {}}
    for nq in args.batches:
        x = queries[:, :nq].contiguous()
        scan32, bytes32 = scan_leg(f32, x)
        scan16, bytes16 = scan_leg(f16, x)
        legs = {"fp32_query_major": lambda: search(f32, x, False), "fp32_cell_major": lambda: search(f32, x, True),
                "fp16_query_major": lambda: search(f16, x, False), "fp16_cell_major": lambda: search(f16, x, True),
                "fp32_scan_kernel": scan32, "fp16_scan_kernel": scan16}
        events = {name: [] for name in legs}
        out = {}
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():          # interleaved: every leg sees the same clocks
                ev, out[name] = timed(fn)
                if step >= args.warmup:
                    events[name].append(ev)
        torch.cuda.synchronize()
        rec = {name: stats([a.elapsed_time(b) for a, b in evs]) for name, evs in events.items()}
        for name, nbytes in (("fp32_scan_kernel", bytes32), ("fp16_scan_kernel", bytes16)):
            rec[name]["scanned_bytes"] = nbytes
            rec[name]["scanned_gbytes_per_s"] = round(nbytes / (rec[name]["median_ms"] * 1e-3) / 1e9, 1)
        for a, b in (("fp32_query_major", "fp16_query_major"), ("fp32_scan_kernel", "fp16_scan_kernel"),
                     ("fp32_cell_major", "fp16_query_major"), ("fp16_query_major", "fp16_cell_major"),
                     ("fp32_cell_major", "fp16_cell_major")):
            rec[f"ratio_{a}_over_{b}"] = round(rec[a]["median_ms"] / rec[b]["median_ms"], 3)
        rec["cell_major_ids_equal_query_major"] = bool(torch.equal(out["fp32_cell_major"][1],
                                                                   out["fp32_query_major"][1]))
        rec["fp16_cell_major_ids_equal_query_major"] = bool(torch.equal(out["fp16_cell_major"][1],
                                                                        out["fp16_query_major"][1]))
        rec["fp16_cell_major_values_equal_query_major"] = bool(torch.equal(
            out["fp16_cell_major"][0].view(torch.int32), out["fp16_query_major"][0].view(torch.int32)))
        rec["candidates_per_query"] = {"fp32_cell_major": candidates(f32, x), "fp16_cell_major": candidates(f16, x)}
        rec["topk_id_overlap_fp16_with_fp32"] = recall(out["fp16_query_major"][1], out["fp32_query_major"][1])
        result["batches"][str(nq)] = rec
        del out
    f32.use_cell_major = f16.use_cell_major = False
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
