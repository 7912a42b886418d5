"""The inputs of the IVFPQ filtered-search GPU tests (tests/test_gpu_ivfpq_filtered.py), generated on the CPU so that
tests/test_ivfpq_filtered_cpu.py can assert their conditions on the oracle alone: for each case some query gets fewer
than k results, some query's filtered result differs from its unfiltered top-k, some query has a tie in value across its
k-th place, and the sparse filter row leaves a whole tile of the 300-slot cell empty while another tile of it has hits.
Oracle values are computed once per case and shared.

The inverted lists are those of tests/ivfpq_range_cases.layout -- cells of 0, 1, 63, 64, 65 and 300 slots, a cell running
past the storage, tombstones, planted duplicate codes, a cell listed twice, n_probe_list below, at and beyond max_nprobe,
a query that probes nothing -- with seeds whose capacity is not a multiple of 32.
"""
import functools

import numpy as np

import ivfpq_filtered_oracle as forc
import ivfpq_range_cases as rcases
from oracle import c_oracle
from oracle import ivfpq_oracle as orc

MAX_M = 148          # the largest m tpq_ivfpq_scan_filtered_topk admits (include/torchpq_amd.h)
KS = (1, 10, 100, 1000)
SPLITS = (None, 1, 5, 7)
ROWS = ("ones", "zeros", "single", "sparse", "half")
BIG_CELL = rcases.CELL_SIZES.index(300)
PAD_WORDS = 2        # words of padding behind ceil(n_slots / 32): all ones, never looked at

# (m, ds, table, nq, n_probe, metric): ivfpq_range_cases.PLAIN_CASES with the largest table capped at MAX_M
PLAIN_CASES = [c if c[0] <= MAX_M else (MAX_M,) + c[1:] for c in rcases.PLAIN_CASES]
# (m, ds, tables, nq, n_probe)
RESIDUAL_CASES = list(rcases.RESIDUAL_CASES)


def filter_rows(lay, rng):
    """allowed bool [5, capacity] (ROWS) for a layout, or None when the layout cannot carry them.  Every row also has
    its bits set on the tombstones and on the free slots between the cells: none of these may produce a hit."""
    is_empty = lay["is_empty"]
    cap = len(is_empty)
    at = np.argwhere(lay["cells"] == BIG_CELL)
    if len(at) == 0:
        return None
    start = int(lay["cs"][at[0][0], at[0][1]])
    live = is_empty == 0
    big = np.zeros(cap, bool)
    big[start:start + 300] = True
    tile = lambda t: np.flatnonzero(live & big & (np.arange(cap) >= start + 64 * t) & (np.arange(cap) < start + 64 * t + 64))
    if len(tile(0)) == 0 or len(tile(2)) == 0:
        return None
    rows = np.zeros((len(ROWS), cap), bool)
    rows[0] = True
    rows[2, rng.choice(tile(2))] = True
    rows[3] = rng.random(cap) < 0.03
    rows[3, start + 64:start + 128] = False          # tile 1 of the 300-slot cell: nothing allowed
    rows[3, rng.choice(tile(0))] = True              # tile 0: at least one hit
    rows[4] = rng.random(cap) < 0.5
    rows[1:] &= live
    rows |= ~live
    return rows, start


def filter_bits(allowed):
    """u32 [n_filters, ceil(capacity / 32) + PAD_WORDS]: the padding, and the bits of the last word beyond the
    capacity, are set"""
    n_filters, cap = allowed.shape
    padded = np.ones((n_filters, ((cap + 31) // 32 + PAD_WORDS) * 32), bool)
    padded[:, :cap] = allowed
    return forc.pack_bits(padded)


def runs_of(nq):
    """the filter_of_query of every run: the rows cycle over the queries -- from every row in turn for a small batch --
    and one run passes NULL (row 0, the all-ones row: the unfiltered scan)"""
    rotations = range(len(ROWS)) if nq <= 3 else (3,)
    return [((np.arange(nq) + r) % len(ROWS)).astype(np.int32) for r in rotations] + [None]


def conditions(case):
    """the four conditions of the module docstring, on the oracle's results alone -> dict of bools"""
    *filtered, plain = case["cand"]                   # the last run is the unfiltered one
    fewer = differs = tie = False
    for cand in filtered:
        for k in KS:
            for (s, v), (us, uv) in zip(cand, plain):
                n = int((~np.isnan(v)).sum())
                fewer |= n < k
                order = np.lexsort((s, -v.astype(np.float64)))
                uorder = np.lexsort((us, -uv.astype(np.float64)))
                differs |= not np.array_equal(s[order][:k], us[uorder][:k])
                tie |= n > k and v[order][k - 1] == v[order][k]
    start, sparse = case["big_start"], case["allowed"][3] & (case["is_empty"] == 0)
    tiles = [sparse[start + 64 * t:start + 64 * t + 64].any() for t in range(5)]
    # ... and some query that uses the sparse row does scan that cell
    seen = any(rows[q] == 3 and ((s >= start) & (s < start + 300)).any()
               for rows, cand in zip(case["runs"], filtered) for q, (s, _) in enumerate(cand))
    return dict(fewer=fewer, differs=differs, tie=tie, empty_tile=(not all(tiles)) and any(tiles), sparse_seen=seen)


def _build(seed0, m, nq, n_probe, over, tables):
    """the first seed from seed0 on whose layout has a capacity that is no multiple of 32, carries the filter rows and
    meets conditions()"""
    for seed in range(seed0, seed0 + 200):
        lay = rcases.layout(seed, m, nq, n_probe, over=over)
        if lay["storage"].shape[1] % 32 == 0:
            continue
        rows = filter_rows(lay, lay["rng"])
        if rows is None:
            continue
        case = dict(lay, seed=seed, allowed=rows[0], big_start=rows[1], bits=filter_bits(rows[0]), runs=runs_of(nq))
        tables(case, lay["rng"])
        if all(conditions(case).values()):
            case["want"] = {(r, k): forc.topk(cand, k) for r, cand in enumerate(case["cand"]) for k in KS}
            return case
    raise AssertionError("no seed gives a case that meets its conditions")


@functools.lru_cache(maxsize=None)
def plain_case(m, ds, table, nq, n_probe, metric, over=True):
    def tables(case, rng):
        case["codebook"] = rng.standard_normal((m, ds, 256)).astype(np.float32)
        case["query"] = rng.standard_normal((m * ds, nq)).astype(np.float32)
        case["lut"] = c_oracle.adc_lut(case["query"], case["codebook"], metric)   # the fma chains of tpq_adc_lut
        case["cand"] = [forc.candidates(case["storage"], case["lut"], case["is_empty"], case["allowed"], rows,
                                        case["cs"], case["sz"], case["npl"]) for rows in case["runs"]]
    return _build(3000 * m + 10 * nq + n_probe, m, nq, n_probe, over, tables)


@functools.lru_cache(maxsize=None)
def residual_case(m, ds, tables, nq, n_probe, over=True):
    def fill(case, rng):
        case["codebook"] = (0.5 * rng.standard_normal((m, ds, 256))).astype(np.float32)
        case["query"] = rng.standard_normal((m * ds, nq)).astype(np.float32)
        case["base_sims"] = (-10.0 * rng.random((nq, n_probe))).astype(np.float32)
        case["part1"] = case["part2"] = case["full"] = None
        if tables == "full":
            case["full"] = rng.standard_normal((nq, n_probe, m, 256)).astype(np.float32)
        else:
            case["part1"] = orc.residual_part1(case["query"], case["codebook"])   # the fma chains of tpq_residual_part1
            case["part2"] = rng.standard_normal((case["n_cells"], m, 256)).astype(np.float32)
        case["cand"] = [forc.candidates_residual(case["storage"], case["part1"], case["part2"], case["cells"],
                                                 case["base_sims"], case["is_empty"], case["allowed"], rows,
                                                 case["cs"], case["sz"], case["npl"], full=case["full"])
                        for rows in case["runs"]]
    return _build(9000 * m + 10 * nq + n_probe, m, nq, n_probe, over, fill)
