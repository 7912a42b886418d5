"""A/B of the cell-major scan's threshold form (csrc/scan_cells.hip, `The threshold from group maxima`) against its seeded
form on bench.py's headline workload: the same index and queries in one process, index.use_cell_threshold off and on
alternating, scan time from HIP events around the native call and step time from the host clock around synchronised
searches; then values and ids compared bit for bit, the candidates per query and the chunks in use of both forms read
from one more search's workspace each, and -- step 0 of the form's plan -- the candidate stage on its own over all
probes (first_probe = 0) with thresholds taken from the search's results.
The library is the one TPQ_AMD_LIB names (a tools/build_variant.sh build with other -DTPQ_CELL_THR_PROBES /
-DTPQ_CELL_THR_GROUP), else the product library.

usage: python tools/cell_threshold_ab.py OUT.json [--reps 3] [--steps 15] [--label NAME]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from torchpq_amd import kernels as K  # noqa: E402


def stats(t):
    t = t.float()
    return {"mean": round(float(t.mean()), 1), "p99": float(t.quantile(0.99)), "max": float(t.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--label", default=os.path.basename(os.environ.get("TPQ_AMD_LIB", "product")))
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

    def run(threshold, steps, warmup=3):
        idx.use_cell_threshold = threshold
        for _ in range(warmup):
            idx.search(queries, k=k)
        torch.cuda.synchronize()
        assert scan.last_cell_major() is True and scan.last_cell_threshold() is threshold
        scan.record_events = []
        t0 = time.perf_counter()
        for _ in range(steps):
            v, i = idx.search(queries, k=k)
        torch.cuda.synchronize()
        step_ms = (time.perf_counter() - t0) / steps * 1e3
        ev, scan.record_events = scan.record_events, None
        return float(np.mean([a.elapsed_time(b) for a, b in ev])), step_ms, v, i

    res = {"label": args.label, "scan_ms_seeded": [], "scan_ms_threshold": [], "step_ms_seeded": [],
           "step_ms_threshold": []}
    for _ in range(args.reps):
        a, sa, v0, i0 = run(False, args.steps)
        b, sb, v1, i1 = run(True, args.steps)
        res["scan_ms_seeded"].append(round(a, 4))
        res["scan_ms_threshold"].append(round(b, 4))
        res["step_ms_seeded"].append(round(sa, 4))
        res["step_ms_threshold"].append(round(sb, 4))
    res["equal_bits"] = bool(torch.equal(v0.view(torch.int32), v1.view(torch.int32)) and torch.equal(i0, i1))
    scan.keep_workspace = True
    for name, threshold in (("seeded", False), ("threshold", True)):
        idx.use_cell_threshold = threshold
        idx.search(queries, k=k)
        torch.cuda.synchronize()
        # [flags][bands][16 chunks of keys and indices][eviction words] | [256 bytes][thresholds][scales][norms][counts]
        lists = 2 * align(nq * 4) + nq * 16 * 512 + align(nq * 16 * 4)
        off = lists + 256 + 3 * align(nq * 4)
        cnt = scan.last_workspace[off:off + 4 * nq].view(torch.int32).clone()
        seed_chunks = 0 if threshold else (k + 63) // 64
        res["queries_redone_exactly_" + name] = scan.last_redone(nq)
        res["candidates_per_query_" + name] = stats(cnt)
        res["chunks_in_use_" + name] = stats(seed_chunks + (cnt.clamp(max=(16 - seed_chunks) * 64) + 63) // 64)
    scan.keep_workspace = False
    scan.last_workspace = None
    # step 0: the candidate stage over all probes with thresholds from the search
    _, cells, npl = idx.probe(queries)
    cs, sz = idx._cell_start[cells].contiguous(), idx._cell_size[cells].contiguous()
    common = (idx._storage, queries, idx.pq_codec.codebook, cells, n_cells, cs, sz, npl)
    emp = idx._is_empty if idx._has_holes else None
    tau = v1[:, k - 1].contiguous()
    cand = K.CellCandidatesHip()
    ms = []
    for it in range(8):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        c0 = cand(*common, tau, first_probe=0, capacity=1024, is_empty=emp)[0]
        e1.record()
        torch.cuda.synchronize()
        if it >= 3:
            ms.append(e0.elapsed_time(e1))
    res["step0_candidate_stage_all_probes_ms"] = {
        "what": "prep, seed, inversion, norms and candidates of probes [0, 32) with tau = the search's k-th value, "
                "wrapper allocations included", "mean": round(float(np.mean(ms)), 4), "min": round(float(np.min(ms)), 4),
        "candidates_per_query": stats(c0)}
    print(json.dumps(res))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
