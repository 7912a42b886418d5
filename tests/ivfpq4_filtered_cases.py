"""The inputs of the IVFPQ4 filtered-search GPU tests (tests/test_gpu_ivfpq4_filtered.py), generated on the CPU so that
tests/test_ivfpq4_filtered_cpu.py can assert their conditions on the oracle alone.

A case is tests/ivfpq4_residual_cases.case -- the lists of tests/ivfpq4_cases.case (cells of 0, 1, 63, 64, 65, 300, 17
and 128 slots, junk in the free slots, duplicated codes, tombstones, one duplicated probe, n_probe_list below, at and
beyond max_nprobe) plus the probed cells and a centroid per cell, so one case serves plain and residual codes -- with
the five filter rows of tests/ivfpq_filtered_cases.filter_rows: ones, zeros, single, sparse (tile 1 of the 300-slot cell
emptied) and half, bits set on tombstones and free slots, the padding words and the bits beyond the capacity all ones.
The runs of filter_of_query are ivfpq_filtered_cases.runs_of(nq).  Seeds are searched from 1000 m + 10 nq + n_probe until
the capacity is no multiple of 32 and the five conditions of ivfpq_filtered_cases.conditions hold: some query gets fewer
than k results, some filtered result differs from the unfiltered one, some query has a tie in value across its k-th
place, the sparse row leaves a tile of the 300-slot cell empty next to one with hits, and a query that uses the sparse
row scans that cell.  Oracle results are computed once per case, at full depth, and shared: a top-k is their prefix.
"""
import functools

import numpy as np

import ivfpq4_filtered_oracle as forc
import ivfpq4_residual_cases as rcases
import ivfpq_filtered_cases as fcases

KS = (1, 10, 100, 1024)
SPLITS = (None, 1, 5, 7)
ROWS = fcases.ROWS

# (m, ds, nq, n_probe, distance): m = 8 one word; 24 two + one tail words; 56 four + two + one; 64 one full unroll; 256
# four, and with n_probe = 8 four groups of two tables; every ds of {1, 2, 5}, n_probe of {1, 4, 8}, both metrics;
# nq = 1000 is the unsplit automatic route
KERNEL_CASES = [
    (8, 1, 1, 1, "euclidean"),
    (8, 2, 3, 8, "inner"),
    (24, 2, 3, 4, "euclidean"),
    (56, 5, 1, 8, "inner"),
    (64, 2, 3, 8, "euclidean"),
    (64, 1, 3, 4, "inner"),
    (256, 1, 3, 8, "euclidean"),
    (8, 2, 1000, 8, "euclidean"),
]


def full_depth(c, rows, distance, residual, with_empty=True):
    """the oracle's whole sorted list of every query under the rows `rows` (None: row 0): (values, address), padded"""
    depth = max(2 * c["storage"].shape[1], max(KS))
    extra = dict(centroids=c["centroids"], cells=c["cells"]) if residual else {}
    return forc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"] if with_empty else None, c["allowed"],
                          rows, c["cs"], c["sz"], c["npl"], depth, distance, **extra)


def _candidates(full):
    v, a = full
    return [(a[q][a[q] >= 0], v[q][a[q] >= 0]) for q in range(len(a))]


@functools.lru_cache(maxsize=None)
def case(m, ds, nq, n_probe, distance, residual):
    for seed in range(1000 * m + 10 * nq + n_probe, 1000 * m + 10 * nq + n_probe + 200):
        c = rcases.case(seed, m, ds, nq, n_probe)
        if c["storage"].shape[1] % 32 == 0:
            continue
        rows = fcases.filter_rows(c, np.random.default_rng(seed + 7))
        if rows is None:
            continue
        c.update(seed=seed, allowed=rows[0], big_start=rows[1], bits=fcases.filter_bits(rows[0]),
                 runs=fcases.runs_of(nq))
        c["full"] = [full_depth(c, run, distance, residual) for run in c["runs"]]
        c["cand"] = [_candidates(full) for full in c["full"]]
        if all(fcases.conditions(c).values()):
            return c
    raise AssertionError("no seed gives a case that meets its conditions")


def want(c, run, k):
    v, a = c["full"][run]
    return np.ascontiguousarray(v[:, :k]), np.ascontiguousarray(a[:, :k])


def mixed_table_case():
    """Residual codes, every slot holding the same code, so a value depends on the probe's centroid alone
    (test_gpu_ivfpq4_residual.test_every_tile_is_looked_up_in_its_own_probes_table), with two filter rows: row 0 allows
    8 to 12 live slots in every cell (all of a cell with fewer) -- a wave's pending slots then come from several
    probes of one group of tables --, row 1 only tiles 0 and 4 of the 300-slot cell: a part that begins inside a cell."""
    c = rcases.case(5, 16, 2, 3, 8, tomb=40, dup=False)
    c["storage"][:] = c["storage"][:, :1]
    rng = np.random.default_rng(55)
    cap = c["storage"].shape[1]
    live = c["is_empty"] == 0
    allowed = np.zeros((2, cap), bool)
    for start, size in {(int(s), int(z)) for s, z in zip(c["cs"].ravel(), c["sz"].ravel())}:
        at = start + np.flatnonzero(live[start:start + size])
        allowed[0, rng.choice(at, min(len(at), int(rng.integers(8, 13))), replace=False)] = True
    big = int(c["cs"][c["sz"] == 300][0])
    allowed[1, big:big + 64] = allowed[1, big + 256:big + 300] = True
    allowed[1] &= live
    allowed |= ~live                                   # bits on the tombstones and the free slots: never a result
    c.update(allowed=allowed, bits=fcases.filter_bits(allowed), big_start=big)
    return c
