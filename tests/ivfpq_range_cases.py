"""The inputs of the IVFPQ range-search GPU tests (tests/test_gpu_ivfpq_range.py), generated on the CPU so that
tests/test_ivfpq_range_cpu.py can assert their conditions on the oracle alone (the pattern of
tests/test_scan_band_inputs_cpu.py): for each case some query has no hit, some query with candidates has every
candidate a hit, and there are hits at all.  Oracle values are computed once per case and shared.
"""
import functools

import numpy as np

import ivfpq_range_oracle as rorc
from oracle import c_oracle
from oracle import ivfpq_oracle as orc

# cells of 0, 1, 63, 64, 65 and about 300 slots (and two more), each with spare capacity behind it -- the layout of
# tests/test_gpu_ivfflat.py::_case -- and a ninth cell at the end of the storage whose extent runs past n_slots
CELL_SIZES = (0, 1, 63, 64, 65, 300, 17, 128)
OVER_INSIDE, OVER_SIZE = 40, 100     # the last cell: 40 slots inside the storage, a size of 100

SPLITS = (None, 1, 5, 7)

# (m, ds, table, nq, n_probe, metric)
PLAIN_CASES = [
    (4, 1, "fused", 3, 4, "euclidean"),            # a single row word
    (12, 2, "fused", 1, 8, "inner"),               # three row words: the loop tail alone
    (16, 4, "fused", 1000, 8, "euclidean"),        # one full group; many workgroups
    (20, 8, "materialised", 3, 8, "euclidean"),    # group + tail; ds above the fused limit
    (64, 2, "fused", 1, 8, "euclidean"),           # the headline code width; 13 tiles over up to 56 waves
    (64, 2, "materialised", 1000, 1, "inner"),
    (156, 1, "fused", 3, 8, "euclidean"),          # the largest table: LDS at its limit
]

# (m, ds, tables, nq, n_probe): part1 given, part1 built in the workgroup, one full table per (query, probe)
RESIDUAL_CASES = [(m, ds, tables, nq, 8) for m, ds, tables in ((8, 4, "part1"), (64, 2, "built"), (16, 8, "full"))
                  for nq in (1, 3)] + [(8, 4, "part1", 1000, 4)]


def layout(seed, m, nq, n_probe, tomb=25, dup=True, over=True):
    """storage of random code bytes with planted duplicates (ties sit on thresholds), tombstones inside the cells, one
    cell listed twice in a row, the cell that leaves the storage probed by query 0, n_probe_list below, at and beyond
    max_nprobe and, from three queries on, a last query that probes nothing.  over=False keeps the last cell inside the
    storage (for the kernels that do not cut a cell: the top-k scan of the cross-check)"""
    rng = np.random.default_rng(seed)
    sizes = np.array(CELL_SIZES, np.int64)
    caps = sizes + rng.integers(1, 9, len(sizes))
    start = (np.cumsum(caps) - caps).astype(np.int64)
    cap = int(caps.sum()) + OVER_INSIDE
    start = np.append(start, cap - OVER_INSIDE)
    sizes = np.append(sizes, OVER_SIZE if over else OVER_INSIDE)
    n_cells = len(sizes)
    storage = rng.integers(0, 256, (m // 4, cap, 4), dtype=np.uint8)      # free slots hold junk
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:min(start[c] + sizes[c], cap)] = 0
    live = np.flatnonzero(is_empty == 0)
    if dup:   # a third of the slots hold one of five codes
        src = rng.choice(live, 5, replace=False)
        dst = rng.choice(live, len(live) // 3, replace=False)
        storage[:, dst] = storage[:, src[rng.integers(0, 5, len(dst))]]
    if tomb:
        is_empty[rng.choice(live, tomb, replace=False)] = 1
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    if n_cells - 1 not in cells[0]:
        cells[0, -1] = n_cells - 1
    if n_probe > 1 and nq > 1:
        cells[1, 1] = cells[1, 0]                       # one cell listed twice in a row: scanned once
    npl = rng.integers(0, n_probe + 3, nq).astype(np.int64)   # below, at and beyond max_nprobe
    npl[:max(1, nq // 2)] = n_probe
    if nq >= 3:
        npl[-1] = 0
    return dict(storage=storage, is_empty=is_empty, cells=cells, cs=start[cells], sz=sizes[cells], npl=npl, rng=rng,
                n_cells=n_cells)


def thresholds(cand, rotate=0):
    """per-query thresholds taken from the query's own candidate values, so most sit exactly ON a value: by turns the
    smallest value (every candidate is a hit), one ulp above the largest (no hit), the median, the upper decile"""
    thr = np.zeros(len(cand), np.float32)
    for q, (_, v) in enumerate(cand):
        v = np.sort(v[~np.isnan(v)])
        if len(v) == 0:
            continue
        kind = (q + rotate) % 4
        thr[q] = (v[0], np.nextafter(v[-1], np.float32(np.inf)), v[len(v) // 2], v[(9 * len(v)) // 10])[kind]
    return thr


def _finish(case, nq):
    """the threshold runs of a case and what the oracle says for each: one run of per-query thresholds, or -- a single
    query cannot both have no hit and have every candidate hit -- three runs of the one query"""
    cand = case["cand"]
    case["n_cand"] = np.array([int((~np.isnan(v)).sum()) for _, v in cand])
    case["runs"] = [thresholds(cand, r) for r in ((0,) if nq > 1 else (0, 1, 2))]
    case["want"] = [rorc.hits(cand, thr) for thr in case["runs"]]
    return case


@functools.lru_cache(maxsize=None)
def plain_case(m, ds, table, nq, n_probe, metric, over=True):
    case = layout(1000 * m + 10 * nq + n_probe, m, nq, n_probe, over=over)
    rng = case["rng"]
    case["codebook"] = rng.standard_normal((m, ds, 256)).astype(np.float32)
    case["query"] = rng.standard_normal((m * ds, nq)).astype(np.float32)
    case["lut"] = c_oracle.adc_lut(case["query"], case["codebook"], metric)   # the fma chains of tpq_adc_lut
    case["cand"] = rorc.candidates(case["storage"], case["lut"], case["is_empty"], case["cs"], case["sz"],
                                   case["npl"])
    return _finish(case, nq)


@functools.lru_cache(maxsize=None)
def residual_case(m, ds, tables, nq, n_probe, over=True):
    case = layout(7000 * m + 10 * nq + n_probe, m, nq, n_probe, over=over)
    rng = case["rng"]
    case["codebook"] = (0.5 * rng.standard_normal((m, ds, 256))).astype(np.float32)
    case["query"] = rng.standard_normal((m * ds, nq)).astype(np.float32)
    case["base_sims"] = (-10.0 * rng.random((nq, n_probe))).astype(np.float32)
    case["part1"] = case["part2"] = case["full"] = None
    if tables == "full":
        case["full"] = rng.standard_normal((nq, n_probe, m, 256)).astype(np.float32)
    else:
        case["part1"] = orc.residual_part1(case["query"], case["codebook"])   # the fma chains of tpq_residual_part1
        case["part2"] = rng.standard_normal((case["n_cells"], m, 256)).astype(np.float32)
    case["cand"] = rorc.candidates_residual(case["storage"], case["part1"], case["part2"], case["cells"],
                                            case["base_sims"], case["is_empty"], case["cs"], case["sz"], case["npl"],
                                            full=case["full"])
    return _finish(case, nq)


def assert_not_vacuous(case, nq):
    """the condition on a case's inputs, asserted on the oracle alone: a query with zero hits, a query whose every live
    candidate is a hit (and that has candidates), hits at all; with one query, by its three runs -- and the third run
    (the median) is a proper subset"""
    n_cand = case["n_cand"]
    hits = np.stack([np.diff(w[0]) for w in case["want"]])
    if nq > 1:
        h, n = hits[0], n_cand
    else:
        h, n = hits[:, 0], np.repeat(n_cand, 3)
        assert 0 < hits[2, 0] < n_cand[0], (hits, n_cand)
    assert (h == 0).any() and ((h == n) & (n > 0)).any() and h.sum() > 0, (h, n)
