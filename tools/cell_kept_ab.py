"""A/B of builds on bench.py's headline workload, for the cell-major scan's kept state, block pieces and inversion
(csrc/scan_cells.hip: `The kept state`, launch_cell_threshold's one walk; csrc/scan_cells.h: TPQ_CELL_PIECES_A, _B).
Each build is a library file -- a tools/build_variant.sh build of scan_cells with other -DTPQ_CELL_PIECES_A/_B, or the
product library -- run through this tree's bench.py, or a DIRECTORY: a built checkout (the parent commit's), whose own
bench.py and package are run: the kept state lives in the index, so the parent is measured whole.  The FIRST build named
is the baseline.
  * step time: `bench.py --gpus 1 --steps S --warmup W` per build in a process of its own (TPQ_AMD_LIB), the builds
    alternating --reps times in one chain; per build the runs, against the baseline the mean gain, the gain over the
    baseline's spread (max - min of its runs) and whether every run is faster than every run of the baseline;
  * kernel time: the same command under `rocprofv3 --kernel-trace --stats` (no counters), --traces times per build; per
    kernel the launches and the summed duration per search, and their sum over the scan's kernels; the baseline's
    trace-to-trace variation is the difference between its sums.
A child that fails ends the chain there: nothing more is started.

usage: python tools/cell_kept_ab.py OUT.json parent=LIB_OR_DIR tree=LIB_OR_DIR [name=...] [--reps 3] [--traces 2]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bench(lib, steps, warmup, prefix=(), timeout=300):
    root, env = ROOT, dict(os.environ)
    if os.path.isdir(lib):
        root = os.path.abspath(lib)
        env.pop("TPQ_AMD_LIB", None)
    else:
        env["TPQ_AMD_LIB"] = os.path.abspath(lib)
    cmd = [*prefix, sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
           str(warmup)]
    out = subprocess.run(cmd, env=env, cwd=root, capture_output=True, text=True, timeout=timeout, check=True).stdout
    line = [ln for ln in out.splitlines() if ln.startswith("{")][-1]
    return json.loads(line)["ms_per_step"]


def trace(lib, steps, warmup):
    """per kernel of the scan: launches and microseconds per search, from one rocprofv3 trace of bench.py"""
    with tempfile.TemporaryDirectory() as td:
        step = bench(lib, steps, warmup, ("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", td,
                                          "-o", "run", "--"))
        rows = []
        for name in glob.glob(os.path.join(td, "**", "*kernel_stats.csv"), recursive=True):
            with open(name) as f:
                rows += list(csv.DictReader(f))
    n = steps + warmup
    kernels = {r["Name"].split("(")[0].replace("void ", ""): {
        "launches_per_search": round(int(r["Calls"]) / n, 2),
        "us_per_search": round(float(r["TotalDurationNs"]) / 1e3 / n, 1)}
        for r in rows if ("cell_" in r["Name"] or "scan_" in r["Name"]) and int(r["Calls"]) >= n}
    # what ran less than once per search: the kept state's build (cell_prep, cell_book and cell_norm<.., true>, once)
    once = {r["Name"].split("(")[0].replace("void ", ""): {"launches": int(r["Calls"]),
                                                            "us": round(float(r["TotalDurationNs"]) / 1e3, 1)}
            for r in rows if "cell_" in r["Name"] and int(r["Calls"]) < n}
    return {"ms_per_step_traced": step, "less_than_once_per_search": once, "sum_us_per_search": round(sum(v["us_per_search"] for v in kernels.values()), 1),
            "launches_per_search": round(sum(v["launches_per_search"] for v in kernels.values()), 2), "kernels": kernels}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out")
    ap.add_argument("builds", nargs="+", help="NAME=LIBRARY; the first is the baseline")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--traces", type=int, default=2)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    builds = [b.split("=", 1) for b in args.builds]
    res = {"command": f"bench.py --gpus 1 --steps {args.steps} --warmup {args.warmup}", "baseline": builds[0][0],
           "step_ms": {name: [] for name, _ in builds}, "traces": {name: [] for name, _ in builds}}
    for _ in range(args.reps):
        for name, lib in builds:
            res["step_ms"][name].append(bench(lib, args.steps, args.warmup))
    for _ in range(args.traces):
        for name, lib in builds:
            res["traces"][name].append(trace(lib, args.steps, args.warmup))
    base = res["step_ms"][builds[0][0]]
    if base:
        spread = max(base) - min(base)
        res["baseline_spread_ms"] = round(spread, 4)
        res["against_baseline"] = {}
        for name, _ in builds[1:]:
            runs = res["step_ms"][name]
            gain = sum(base) / len(base) - sum(runs) / len(runs)
            res["against_baseline"][name] = {"mean_gain_ms": round(gain, 4),
                                             "gain_over_baseline_spread": round(gain / spread, 1) if spread else None,
                                             "every_run_faster": max(runs) < min(base)}
    sums = [t["sum_us_per_search"] for t in res["traces"][builds[0][0]]]
    if len(sums) > 1:
        res["baseline_trace_variation_us"] = round(max(sums) - min(sums), 1)
    print(json.dumps({k: v for k, v in res.items() if k != "traces"}))
    print(json.dumps({name: [t["sum_us_per_search"] for t in ts] for name, ts in res["traces"].items()}))
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
