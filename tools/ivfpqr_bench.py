#!/usr/bin/env python
"""What the re-rank stage of IVFPQRIndex costs, at a SIFT1M-like shape, through the public API.

Per rerank_factor and per step, interleaved in one process (HIP-event timed, median and spread over the steps):
  (a) IVFPQRIndex.search(k)
  (b) IVFPQIndex.search(k1 = k * rerank_factor) on the same vectors -- the existing first stage, unchanged
  (c) the re-rank entry point alone (IVFPQRerankHip) on the first stage's candidates
  (d) the same re-rank composed from existing pieces, the way the legacy reference does it:
      get_data_by_address -> PQDecodeHip twice -> add -> batched torch similarity -> topk
Prints one JSON line.

    python tools/ivfpqr_bench.py [--n 1000000 --nq 10000 --k 100 --factors 1,2,4 --steps 20 --warmup 3]
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


def composed_rerank(idx, x, cand, k):
    """(d): what a user would write today with the package's existing pieces"""
    nq, k1 = cand.shape
    m = idx.n_subvectors
    codes = idx.get_data_by_address(cand.reshape(-1))
    recon = idx.pq_rerank_codec.decode(codes[m:].contiguous())
    if idx.use_residual:
        recon = recon + idx.pq_codec.decode(codes[:m].contiguous())
    recon = recon.view(idx.d_vector, nq, k1)
    if idx.distance == "euclidean":
        sims = -((x[:, :, None] - recon) ** 2).sum(0)
    else:
        sims = (x[:, :, None] * recon).sum(0)
    sims = sims.masked_fill(cand < 0, float("-inf"))
    vals, pos = sims.topk(k, dim=1)
    address = cand.gather(1, pos)
    return vals, address, idx.get_id_by_address(address)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    return (e0, e1), out


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
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--m-rerank", type=int, default=64)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--factors", default="1,2,4")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

    from torchpq_amd.index import IVFPQIndex, IVFPQRIndex
    from torchpq_amd.kernels import IVFPQRerankHip

    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:args.nq]]
               + 0.3 * torch.randn(args.d, args.nq, device="cuda", generator=gen)).contiguous()
    idx = IVFPQRIndex(args.d, n_subvectors=args.m, n_subvectors_rerank=args.m_rerank, n_cells=args.n_cells,
                      initial_size=max(64, 2 * args.n // args.n_cells))
    idx.train(base[:, :args.n_train].contiguous())
    plain = IVFPQIndex(args.d, n_subvectors=args.m, n_cells=args.n_cells,
                       initial_size=max(64, 2 * args.n // args.n_cells))
    plain.vq_codec.load_state_dict(idx.vq_codec.state_dict())
    plain.pq_codec.load_state_dict(idx.pq_codec.state_dict())
    for b0 in range(0, args.n, 250000):
        idx.add(base[:, b0:b0 + 250000].contiguous())
        plain.add(base[:, b0:b0 + 250000].contiguous())
    idx.release_spare()
    plain.release_spare()
    idx.n_probe = plain.n_probe = args.n_probe
    rerank = IVFPQRerankHip()

    result = {"tool": "ivfpqr_bench", "device": torch.cuda.get_device_name(0), "d": args.d, "n": args.n,
              "n_cells": args.n_cells, "n_probe": args.n_probe, "m": args.m, "m_rerank": args.m_rerank,
              "nq": args.nq, "k": args.k, "steps": args.steps, "warmup": args.warmup, "factors": {}}
    for factor in [int(f) for f in args.factors.split(",")]:
        idx.rerank_factor = factor
        k1 = args.k * factor
        sims, cells, npl = plain.probe(queries)
        _, _, cand = plain.search_cells(x=queries, cells=cells, base_sims=sims, n_probe_list=npl, k=k1,
                                        return_address=True)
        legs = {
            "a_ivfpqr_search": lambda: idx.search(queries, k=args.k),
            "b_ivfpq_search_k1": lambda: plain.search(queries, k=k1),
            "c_rerank_kernel": lambda: rerank(idx._storage, args.m, idx.pq_codec.codebook,
                                              idx.pq_rerank_codec.codebook, queries, cand, args.k,
                                              use_residual=idx.use_residual, distance=idx.distance,
                                              address2id=idx._address2id),
            "d_rerank_composed": lambda: composed_rerank(idx, queries, cand, args.k),
        }
        events = {name: [] for name in legs}
        out = {}
        for step in range(args.warmup + args.steps):
            for name, fn in legs.items():          # interleaved: every leg sees the same clocks
                ev, out[name] = timed(fn)
                if step >= args.warmup:
                    events[name].append(ev)
        torch.cuda.synchronize()
        rec = {name: stats([a.elapsed_time(b) for a, b in evs]) for name, evs in events.items()}
        c_ids, d_ids = out["c_rerank_kernel"][2], out["d_rerank_composed"][2]
        rec["c_vs_d_ids_equal_fraction"] = round(float((c_ids == d_ids).float().mean()), 6)
        rec["a_equals_c_ids"] = bool(torch.equal(out["a_ivfpqr_search"][1], c_ids))
        rec["a_minus_b_ms"] = round(rec["a_ivfpqr_search"]["median_ms"] - rec["b_ivfpq_search_k1"]["median_ms"], 4)
        rec["a_over_b"] = round(rec["a_ivfpqr_search"]["median_ms"] / rec["b_ivfpq_search_k1"]["median_ms"], 4)
        rec["c_over_d"] = round(rec["c_rerank_kernel"]["median_ms"] / rec["d_rerank_composed"]["median_ms"], 4)
        result["factors"][str(factor)] = rec
        del out, cand
        torch.cuda.empty_cache()
    print(json.dumps(result))


if __name__ == "__main__":
    main()
