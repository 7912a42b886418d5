#!/usr/bin/env python
"""What the masked list scan of IVFFlatIndex costs and saves, at the shape of tools/ivfflat_bench.py:
1 M x 128 clustered vectors, 1 024 cells, n_probe = 32, 10 000 queries, k = 100, in one process.

Two indexes hold the same vectors: `full`, and `holed`, from which 1 % of the ids were removed.  `remove` moves a
cell's last items into the holes, so neither index has a tombstone inside a cell and the searches of both run the
unmasked scan; the masked scan at a mask that is 99 % live is therefore measured on the scan launch itself, with 1 %
of `full`'s live slots marked in a copy of its tombstones.  Per step, interleaved (HIP-event timed after warm-up; median,
min, max and the spread (max - min) / median over the steps):
  a_search                full.search(k): the unmasked scan, whose instructions are the parent commit's
  b_search_removed        holed.search(k): after `remove`, still the unmasked scan (`holed_has_holes` is recorded)
  scan_<lib>_<mask>       the scan launch alone on `full` under each mask -- `removed`: the 99 % live one; `allowed_<s>`:
                          the filter rows of the c legs -- through this build's library (`this`) and through every
                          `--lib NAME=PATH` given (`parent`: a library built from the parent commit; others: variants
                          of the masked scan), alternately, same tensors; per mask the results of all libraries are
                          asserted equal bit for bit.  b: scan_this_removed over scan_parent_removed; margin: the
                          larger of the two legs' spreads
  c_filtered_<s>          full.search_filtered(k, flt) with a fraction s of the ids allowed, one row; over a_search
  d_overfetch             full.search(k = 1024) cut by hand to the s = 0.01 id set: the time, and how many of a query's
                          filtered neighbours the cut finds
At s = 1 the filtered result is asserted equal to full.search, bit for bit.  Prints one JSON line and writes it to --out.

    python tools/ivfflat_filtered_bench.py [--lib parent=PATH --steps 10 --warmup 2 --out profiles/ivfflat_filtered_bench.json]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.ivfflat_bench import clustered, stats, timed  # noqa: E402
from tools.ivfpq_filtered_bench import found_by_overfetch, id_subset  # noqa: E402

SELECTIVITIES = (1.0, 0.5, 0.1, 0.01, 0.001)


def spread(leg):
    return round((leg["max_ms"] - leg["min_ms"]) / leg["median_ms"], 4)


def other_scan(path):
    """tpq_ivfflat_scan_topk of another build of the library, with this build's signature (the ABI is unchanged)"""
    from torchpq_amd import _lib
    lib = C.CDLL(os.path.abspath(path))
    fn = lib.tpq_ivfflat_scan_topk
    fn.restype, fn.argtypes = _lib.SIGNATURES["tpq_ivfflat_scan_topk"]
    lib.tpq_last_error.restype = C.c_char_p
    return lib, fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--n-train", type=int, default=100000)
    ap.add_argument("--n-cells", type=int, default=1024)
    ap.add_argument("--n-probe", type=int, default=32)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--removed", type=float, default=0.01, help="fraction of the ids removed from the second index")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--lib", action="append", default=[], metavar="NAME=PATH",
                    help="another build of libtorchpq_amd.so to time the scan launch through (parent=... for b)")
    ap.add_argument("--variant", default=None, help="a label for this build, recorded in the result")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_filtered_bench.json"))
    args = ap.parse_args()

    from torchpq_amd import _lib
    from torchpq_amd.index import IVFFlatIndex
    from torchpq_amd.kernels._common import metric_code

    assert torch.cuda.is_available(), "ivfflat_filtered_bench measures on the GPU; there is nothing to report without one"
    gen = torch.Generator(device="cuda").manual_seed(0)
    np.random.seed(0)
    base = clustered(args.d, args.n, 256, gen)
    nq, k = args.nq, args.k
    queries = (base[:, torch.randperm(args.n, device="cuda", generator=gen)[:nq]]
               + 0.3 * torch.randn(args.d, nq, device="cuda", generator=gen)).contiguous()
    per_cell = max(64, 2 * args.n // args.n_cells)
    full = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=per_cell)
    full.train(base[:, :args.n_train].contiguous())
    holed = IVFFlatIndex(args.d, n_cells=args.n_cells, initial_size=per_cell)
    holed.vq_codec.load_state_dict(full.vq_codec.state_dict())
    for b0 in range(0, args.n, 250000):
        chunk = base[:, b0:b0 + 250000].contiguous()
        full.add(chunk)
        holed.add(chunk)
    del base
    full.release_spare()
    holed.release_spare()
    ids = full._address2id[full._address2id >= 0].contiguous()
    holed.remove(ids=id_subset(ids, args.removed, 7))
    full.n_probe = holed.n_probe = args.n_probe
    assert not full._has_holes

    # the scan launch of `full` alone, as IVFFlatTopkHip makes it, through every library; the `removed` mask skips the
    # free slots and `removed` of the live ones
    g = torch.Generator(device="cuda").manual_seed(11)
    removed = (full._is_empty | (torch.rand(full.capacity, device="cuda", generator=g) < args.removed)).to(torch.uint8)
    _, cells, npl = full.probe(queries)
    cell_start, cell_size = full._cell_start[cells].contiguous(), full._cell_size[cells].contiguous()
    slots_hint = cells.shape[1] * full.capacity // full.n_cells
    full._flat_topk(full._vectors(), queries, cell_start, cell_size, npl, k, is_empty=removed, slots_hint=slots_hint)
    n_split = full._flat_topk.last_n_split
    assert n_split == 1, "a batch this large is one workgroup per query: no workspace"
    libs = {"this": (_lib.load(), _lib.load().tpq_ivfflat_scan_topk)}
    for spec in args.lib:
        name, path = spec.split("=", 1)
        libs[name] = other_scan(path)
    scan_out = {name: (torch.empty(nq, k, device="cuda", dtype=torch.float32),
                       torch.empty(nq, k, device="cuda", dtype=torch.int64)) for name in libs}

    def scan_through(name, mask):
        vectors, (v, a) = full._vectors(), scan_out[name]
        rc = libs[name][1](_lib.ptr(vectors), _lib.ptr(queries), _lib.ptr(mask), _lib.ptr(cell_start),
                           _lib.ptr(cell_size), _lib.ptr(npl), _lib.ptr(v), _lib.ptr(a), vectors.shape[1], args.d, nq,
                           cells.shape[1], k, metric_code(full.distance), 1, None, 0, _lib.stream_ptr("cuda:0"))
        assert rc == 0, libs[name][0].tpq_last_error()
        return v, a

    allowed = {s: id_subset(ids, s, 100) for s in SELECTIVITIES}
    filters = {s: full.id_filter(allowed[s]) for s in SELECTIVITIES}
    build_ms = {}
    for s in SELECTIVITIES:
        ev, _ = timed(lambda: filters[s].masks())         # a row from its ids: the id look-up and the torch ops
        torch.cuda.synchronize()
        build_ms[s] = round(ev[0].elapsed_time(ev[1]), 4)

    def overfetch():
        v, i = full.search(queries, k=1024)
        ok = torch.isin(i, allowed[0.01]) & (i >= 0)
        return v, torch.where(ok, i, torch.full_like(i, -1))

    masks = {"removed": removed, **{f"allowed_{s}": filters[s].masks()[0] for s in SELECTIVITIES}}
    legs = {"a_search": lambda: full.search(queries, k=k),
            "b_search_removed": lambda: holed.search(queries, k=k)}
    for s in SELECTIVITIES:
        legs[f"c_filtered_{s}"] = (lambda s=s: full.search_filtered(queries, k, filters[s]))
    legs["d_overfetch"] = overfetch
    for mname, mask in masks.items():
        for name in libs:
            legs[f"scan_{name}_{mname}"] = (lambda name=name, mask=mask: scan_through(name, mask))
    # per mask, every library gives the same bits
    for mname, mask in masks.items():
        want = tuple(t.clone() for t in scan_through("this", mask))
        for name in libs:
            v, a = scan_through(name, mask)
            assert torch.equal(a, want[1]) and torch.equal(v.view(torch.int32), want[0].view(torch.int32)), (name, mname)
    events = {name: [] for name in legs}
    out = {}
    for step in range(args.warmup + args.steps):
        for name, fn in legs.items():          # interleaved: every leg sees the same clocks
            ev, out[name] = timed(fn)
            if step >= args.warmup:
                events[name].append(ev)
    torch.cuda.synchronize()
    res = {"tool": "ivfflat_filtered_bench", "device": torch.cuda.get_device_name(0), "variant": args.variant,
           "d": args.d, "n": args.n, "n_cells": args.n_cells, "n_probe": args.n_probe, "nq": nq, "k": k,
           "removed": args.removed, "steps": args.steps, "warmup": args.warmup,
           "index_bytes": int(full._storage.numel()), "n_split": n_split,
           "holed_has_holes": bool(holed._has_holes), "b_mask_live_fraction": round(
               float((removed == 0).sum()) / float((full._is_empty == 0).sum()), 5)}
    for name, evs in events.items():
        res[name] = stats([a.elapsed_time(b) for a, b in evs], nq)
        res[name]["spread"] = spread(res[name])
    # every id allowed: search, bit for bit
    assert torch.equal(out["c_filtered_1.0"][1], out["a_search"][1])
    assert torch.equal(out["c_filtered_1.0"][0].view(torch.int32), out["a_search"][0].view(torch.int32))
    res["libs"] = list(libs)
    res["scan_median_ms"] = {name: {m: res[f"scan_{name}_{m}"]["median_ms"] for m in masks} for name in libs}
    if "parent" in libs:
        mine, theirs = res["scan_this_removed"], res["scan_parent_removed"]
        res["b_scan_over_parent"] = round(mine["median_ms"] / theirs["median_ms"], 4)
        res["b_margin"] = max(mine["spread"], theirs["spread"])
        res["b_slower_beyond_margin"] = bool(res["b_scan_over_parent"] > 1 + res["b_margin"])
    res["b_search_removed_over_a"] = round(res["b_search_removed"]["median_ms"] / res["a_search"]["median_ms"], 4)
    res["selectivity"] = {}
    for s in SELECTIVITIES:
        leg = res[f"c_filtered_{s}"]
        row = {"allowed_ids": int(allowed[s].numel()), "mask_build_ms": build_ms[s],
               "over_a_search": round(leg["median_ms"] / res["a_search"]["median_ms"], 4)}
        row["faster_than_a_beyond_spread"] = bool(
            leg["median_ms"] < res["a_search"]["median_ms"] * (1 - max(leg["spread"], res["a_search"]["spread"])))
        res["selectivity"][str(s)] = row
    have, found = found_by_overfetch(out["d_overfetch"][1], allowed[0.01], out["c_filtered_0.01"][1])
    res["d_filtered_neighbours_per_query"] = round(have, 2)
    res["d_found_by_overfetch_1024"] = round(found, 2)
    res["d_over_c_filtered_0.01"] = round(res["d_overfetch"]["median_ms"] / res["c_filtered_0.01"]["median_ms"], 4)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
