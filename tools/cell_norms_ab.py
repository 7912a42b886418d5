"""A/B of the per-call slot norms of the cell-major form (cell_norm_kernel, csrc/scan_cells.hip) on bench.py's headline
workload: the same index and queries in one process, the workspace at exactly lists + extras (the candidate kernel forms
the norms in every block) and at the library's own size (norms once per call) alternating, scan time from HIP events
around the native call; then values and ids compared bit for bit and the candidates per query of both read from one
more search's workspace each.

usage: python tools/cell_norms_ab.py OUT.json [--reps 3] [--steps 15]"""
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
from torchpq_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    args = ap.parse_args()
    device = torch.device("cuda:0")
    nq, k, n_probe, n_cells = 10000, 100, 32, 1024
    synth = bench.SiftLike(128, device)
    base = synth.sample(1_000_000, seed=1)
    gsel = torch.Generator(device=device)
    gsel.manual_seed(2)
    train = base[:, torch.randperm(1_000_000, generator=gsel, device=device)[:100000]].contiguous()
    idx, _, _ = bench.build_index(types.SimpleNamespace(m=64, n_cells=n_cells), device, base, train)
    del base, train
    idx.n_probe = n_probe
    idx.use_smart_probing = False
    queries = synth.sample(nq, seed=4321)
    scan = idx._ivfpq_topk._scan
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    lists = 2 * align(nq * 4) + nq * 16 * 512 + align(nq * 16 * 4)
    no_room = lists + _lib.load().tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, n_cells, 4)

    def run(norms, steps, warmup=3):
        scan.workspace_bytes = None if norms else no_room
        for _ in range(warmup):
            idx.search(queries, k=k)
        torch.cuda.synchronize()
        assert scan.last_cell_major() is True and scan.last_cell_norms() is norms
        scan.record_events = []
        for _ in range(steps):
            v, i = idx.search(queries, k=k)
        torch.cuda.synchronize()
        ev, scan.record_events = scan.record_events, None
        return [a.elapsed_time(b) for a, b in ev], v, i

    res = {"scan_ms_chain": [], "scan_ms_norms": [], "workspace_bytes_chain": no_room}
    for _ in range(args.reps):
        a, v0, i0 = run(False, args.steps)
        b, v1, i1 = run(True, args.steps)
        res["scan_ms_chain"].append(round(float(np.mean(a)), 4))
        res["scan_ms_norms"].append(round(float(np.mean(b)), 4))
    res["workspace_bytes_norms"] = scan.last_workspace_bytes
    res["equal_bits"] = bool(torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1))
    scan.keep_workspace = True
    counts = {}
    for name, norms in (("chain", False), ("norms", True)):
        scan.workspace_bytes = None if norms else no_room
        idx.search(queries, k=k)
        torch.cuda.synchronize()
        # [flags][bands][lists][eviction words] | [256 bytes][thresholds][scales][norms][candidate counts] (csrc/scan_cells.h)
        off = lists + 256 + 3 * align(nq * 4)
        cnt = scan.last_workspace[off:off + 4 * nq].view(torch.int32).clone()
        counts[name] = cnt
        res["queries_redone_exactly_" + name] = scan.last_redone(nq)
        c = cnt.float()
        res["candidates_per_query_" + name] = {"mean": round(float(c.mean()), 1), "p99": float(c.quantile(0.99)),
                                               "max": float(c.max())}
    res["candidate_counts_equal"] = bool(torch.equal(counts["chain"], counts["norms"]))
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
