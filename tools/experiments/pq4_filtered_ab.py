#!/usr/bin/env python
"""The two A/Bs of scan_pq4_filtered_residual_kernel that DESIGN 3.16 records (measured, not kept), repeated on the legs
of tools/ivfpq4_filtered_bench.py, interleaved with them in the same process, and recorded under "ab" in the same profile.

Needs the kernel of tools/experiments/pq4_filtered_ab.patch (patched into a copy of torchpq_amd/csrc that keeps include/
two levels above it, as in the tree) built as a variant:
    SRC_DIR=<that copy> tools/build_variant.sh ab "" scan_pq4_filtered
    TPQ_AMD_LIB=torchpq_amd/variants/libtorchpq_amd_ab.so python tools/experiments/pq4_filtered_ab.py
In that build the residual kernel runs WITH probe skipping (a membership pass ahead of the group walk; no table for a
probe without an allowed live slot) unless TPQ_PQ4F_NO_PROBE_SKIP=1, and drains a wave's pending slots whenever its
tiles change probe (no batch mixes tables) when TPQ_PQ4F_DRAIN_PER_PROBE=1 -- environment variables only such a build
reads.  Per residual index and selectivity, shared row, four forms:
  skip              probe skipping, drain per group (the variant's default)
  noskip            no skipping, drain per group: the product's form
  perprobe          probe skipping, drain per probe
  noskip_perprobe   no skipping, drain per probe: the mixed-table question against the product's form
Every form's result is asserted equal to the first's, bit for bit.
"""
import contextlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools import ivfpq4_filtered_bench as bench  # noqa: E402
from tools.ivfpq_filtered_bench import SELECTIVITIES  # noqa: E402

SKIP, DRAIN = "TPQ_PQ4F_NO_PROBE_SKIP", "TPQ_PQ4F_DRAIN_PER_PROBE"
FORMS = {"skip": (), "noskip": (SKIP,), "perprobe": (DRAIN,), "noskip_perprobe": (SKIP, DRAIN)}


@contextlib.contextmanager
def switched(names):
    for n in names:
        os.environ[n] = "1"
    try:
        yield
    finally:
        for n in names:
            del os.environ[n]


class Forms:
    def legs(self, idx, queries, k, shared):
        legs = {}
        for form, names in FORMS.items():
            for s in SELECTIVITIES:
                def leg(s=s, names=names):
                    with switched(names):
                        return idx.search_filtered(queries, k, shared[s])
                legs[f"ab_{form}_{s}"] = leg
        return legs

    def finish(self, res, out):
        table = {}
        for s in SELECTIVITIES:
            ref = out[f"ab_skip_{s}"]
            row = {}
            for form in FORMS:
                got = out[f"ab_{form}_{s}"]
                assert torch.equal(got[1], ref[1]) and torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
                row[form] = res.pop(f"ab_{form}_{s}")
            row["skip_over_noskip"] = round(row["skip"]["median_ms"] / row["noskip"]["median_ms"], 4)
            row["noskip_perprobe_over_noskip"] = round(
                row["noskip_perprobe"]["median_ms"] / row["noskip"]["median_ms"], 4)
            table[str(s)] = row
        res["ab"] = table


def main():
    ap = bench.parser()
    ap.set_defaults(only="residual_1024,residual_16384", label="tools/experiments/pq4_filtered_ab.patch variant")
    args = ap.parse_args()
    assert os.environ.get("TPQ_AMD_LIB"), "the switches exist only in a tools/build_variant.sh library"
    assert not (os.environ.get(SKIP) or os.environ.get(DRAIN)), "this script sets the switches itself"
    result = bench.run(args, Forms())
    record = {key: result[key] for key in ("label", "library", "device", "steps", "warmup")}
    for name in args.only.split(","):
        record[name] = {"search_k100": result[name]["search_k100"], "forms": result[name]["ab"]}
    print(json.dumps(record))
    if args.out:       # into the bench's own profile, next to the product's numbers
        profile = json.load(open(args.out)) if os.path.exists(args.out) else {}
        profile["ab"] = record
        with open(args.out, "w") as f:
            f.write(json.dumps(profile) + "\n")


if __name__ == "__main__":
    main()
