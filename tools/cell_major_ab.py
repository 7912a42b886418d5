"""A/B of the cell-major form of the m = 64 large-batch scan route (csrc/scan_cells.hip) on bench.py's headline workload:
the same index and queries, `index.use_cell_major` off / on alternating, scan time from HIP events around the native call;
then the candidates per query, the band and the redo count read from one more search's workspace.

usage: python tools/cell_major_ab.py OUT.json [--reps 3] [--steps 15] [--profile on|off]
  --profile: a few searches in one mode and nothing else (the command to put behind `rocprofv3 --kernel-trace --stats --`)
TPQ_AMD_LIB=<variant library> measures a build with another P0 (-DTPQ_CELL_P0=n for scan.hip and scan_cells.hip)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--profile", choices=["on", "off"], default=None)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    nq, k = 10000, 100
    synth = bench.SiftLike(128, device)
    base = synth.sample(1_000_000, seed=1)
    gsel = torch.Generator(device=device)
    gsel.manual_seed(2)
    train = base[:, torch.randperm(1_000_000, generator=gsel, device=device)[:100000]].contiguous()
    idx, _, _ = bench.build_index(types.SimpleNamespace(m=64, n_cells=1024), device, base, train)
    del base, train
    idx.n_probe = 32
    idx.use_smart_probing = False
    queries = synth.sample(nq, seed=4321)
    scan = idx._ivfpq_topk._scan

    def run(on, steps, warmup=3):
        idx.use_cell_major = on
        for _ in range(warmup):
            idx.search(queries, k=k)
        torch.cuda.synchronize()
        scan.record_events = []
        for _ in range(steps):
            v, i = idx.search(queries, k=k)
        torch.cuda.synchronize()
        ev, scan.record_events = scan.record_events, None
        return [a.elapsed_time(b) for a, b in ev], v, i

    if args.profile:
        run(args.profile == "on", 5, 2)
        return
    res = {"lib": os.environ.get("TPQ_AMD_LIB", "built"), "scan_ms_off": [], "scan_ms_on": []}
    for _ in range(args.reps):
        a, v0, i0 = run(False, args.steps)
        b, v1, i1 = run(True, args.steps)
        res["scan_ms_off"].append(round(float(np.mean(a)), 4))
        res["scan_ms_on"].append(round(float(np.mean(b)), 4))
        res["form_taken"] = scan.last_cell_major()
    res["equal_bits"] = bool(torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1))
    scan.keep_workspace = True
    idx.use_cell_major = True
    idx.search(queries, k=k)
    torch.cuda.synchronize()
    res["queries_redone_exactly"] = scan.last_redone(nq)
    ws = scan.last_workspace
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    # the workspace of the form: [flags][bands][16 chunks of 64 keys per query, twice][eviction words][256 bytes of
    # constants][thresholds][scales][norms][candidate counts] ... (csrc/scan_cells.h)
    lists = 2 * align(nq * 4) + nq * 16 * 512 + align(nq * 16 * 4)
    off = lists + 256 + 3 * align(nq * 4)
    cnt = ws[off:off + 4 * nq].view(torch.int32).float()
    res["candidates_per_query"] = {"mean": round(float(cnt.mean()), 1), "p99": float(cnt.quantile(0.99)),
                                   "max": float(cnt.max())}
    band = ws[align(nq * 4):align(nq * 4) + 4 * nq].view(torch.float32)
    res["band_mean"] = float(band.mean())
    res["kth_value_mean"] = float(v1[:, -1].mean())
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
