"""The inputs of the IVFPQ4 range-search GPU tests (tests/test_gpu_ivfpq4_range.py), generated on the CPU so that
tests/test_ivfpq4_range_cpu.py can assert their conditions on the oracle alone.

A case is tests/ivfpq4_filtered_cases.case -- cells of 0, 1, 63, 64, 65, 300, 17 and 128 slots, junk in the free slots,
tombstones, one duplicated probe, n_probe_list below, at and beyond max_nprobe, a capacity that is no multiple of 32,
the probed cells and a centroid per cell (one case serves plain and residual codes), five filter rows (ones, zeros,
single, sparse, half) and the runs of filter_of_query -- on its KERNEL_CASES.  The candidates of a case (oracle values,
scan order) are computed once per (codes, filter run, tombstones) and kept in the case; every threshold is applied to
them.

Thresholds come from the candidates' values, per query: the median; a candidate's own value (the boundary is a hit);
that value's next float up (it is not); and -inf, +inf and NaN mixed across the queries of one call (with one query,
one call each).
"""
import numpy as np

import ivfpq4_filtered_cases as fcases
import ivfpq4_range_oracle as rgo

KERNEL_CASES = fcases.KERNEL_CASES
SPLITS = fcases.SPLITS
ROWS = fcases.ROWS
WAVES = 8


def case(m, ds, nq, n_probe, distance, residual):
    return fcases.case(m, ds, nq, n_probe, distance, residual)


def candidates(c, residual, distance, run=None, with_empty=True, probes=False):
    """the oracle's candidates of the case under filter run `run` (an index into c["runs"]; None: no filter), cached
    in the case"""
    key = ("range_cand", bool(residual), distance, run, with_empty, probes)
    if key not in c:
        extra = dict(centroids=c["centroids"], cells=c["cells"]) if residual else {}
        flt = {} if run is None else dict(allowed=c["allowed"], rows=c["runs"][run])
        c[key] = rgo.candidates(c["storage"], c["query"], c["codebook"], c["is_empty"] if with_empty else None,
                                c["cs"], c["sz"], c["npl"], distance, probes=probes, **extra, **flt)
    return c[key]


def _ranked(v):
    """the candidate values that are not NaN, descending"""
    v = v[~np.isnan(v)]
    return np.sort(v)[::-1]


def thresholds(cand):
    """name -> f32 [nq], from the candidates' own values"""
    nq = len(cand)
    median, boundary = np.zeros(nq, np.float32), np.zeros(nq, np.float32)
    for q, (_, v) in enumerate(cand):
        r = _ranked(v)
        if len(r):
            median[q] = r[len(r) // 2]
            boundary[q] = r[len(r) // 3]
    with np.errstate(over="ignore"):
        above = np.nextafter(boundary, np.float32(np.inf)).astype(np.float32)
    out = dict(median=median, boundary=boundary, above=above)
    special = [np.float32(-np.inf), np.float32(np.inf), np.float32(np.nan)]
    if nq == 1:
        for i, name in enumerate(("minus_inf", "plus_inf", "nan")):
            out[name] = np.array([special[i]], np.float32)
    else:
        for r in range(3 if nq <= 3 else 1):
            t = median.copy()
            for q in range(nq):
                i = (q + r) % 4
                if i < 3:
                    t[q] = special[i]
            out["mixed%d" % r] = t
    return out


def boundary_exists(cand, thr):
    """per query with candidates: the boundary threshold equals some candidate's value"""
    return all(len(_ranked(v)) == 0 or (v == thr["boundary"][q]).any() for q, (_, v) in enumerate(cand))


# ---- the segments: which wave counts which hit ---------------------------------------------------------------------
def _scanned(c, q):
    """the probes query q scans: [(rank, start, size)]"""
    n = int(min(max(int(c["npl"][q]), 0), c["cs"].shape[1]))
    return [(p, int(c["cs"][q, p]), int(c["sz"][q, p])) for p in range(n)
            if c["sz"][q, p] > 0 and not (p > 0 and c["cs"][q, p] == c["cs"][q, p - 1])]


def segment_counts(c, cand_p, threshold, residual, n_split=1):
    """the wave_counts of the count pass, from the oracle's candidates with their probe ranks (candidates(...,
    probes=True)): plain codes i32 [nq, n_split, 8] -- a query's tiles cut into n_split parts, a part's into eight
    contiguous chunks --, residual codes i32 [nq, max_nprobe, 8] -- the tiles of one probe in eight contiguous chunks"""
    nq, max_nprobe = c["cs"].shape
    out = np.zeros((nq, max_nprobe if residual else n_split, WAVES), np.int32)
    threshold = np.broadcast_to(np.asarray(threshold, np.float32), (nq,))
    for q, (s, v, p) in enumerate(cand_p):
        with np.errstate(invalid="ignore"):
            hit = v >= threshold[q]
        s, p = s[hit], p[hit]
        probes = _scanned(c, q)
        first, total = {}, 0
        for rank, start, size in probes:                 # the first tile of every scanned probe, query-wide
            first[rank] = total
            total += (size + 63) // 64
        start_of = {rank: start for rank, start, _ in probes}
        size_of = {rank: size for rank, _, size in probes}
        for slot, rank in zip(s, p):
            t_in = (int(slot) - start_of[int(rank)]) // 64
            if residual:
                n = (size_of[int(rank)] + 63) // 64
                wave = next(w for w in range(WAVES) if n * w // WAVES <= t_in < n * (w + 1) // WAVES)
                out[q, int(rank), wave] += 1
            else:
                T = first[int(rank)] + t_in
                part = next(g for g in range(n_split) if total * g // n_split <= T < total * (g + 1) // n_split)
                b, e = total * part // n_split, total * (part + 1) // n_split
                n = e - b
                wave = next(w for w in range(WAVES) if b + n * w // WAVES <= T < b + n * (w + 1) // WAVES)
                out[q, part, wave] += 1
    return out


def overlap_case():
    """Residual codes, one query, two probes whose cells OVERLAP: probe 0 scans [start, start + 100) of the 300-slot
    cell's storage under one cell's centroid, probe 1 scans [start + 40, start + 140) under another's -- sixty slots are
    scanned twice, each time in its own probe's table"""
    c = dict(fcases.case(24, 2, 3, 4, "euclidean", True))
    for k in [k for k in c if k == "gpu" or (isinstance(k, tuple) and k[0] == "range_cand")]:
        c.pop(k)
    big = int(c["big_start"])
    c["query"] = np.ascontiguousarray(c["query"][:, :1])
    c["cs"] = np.array([[big, big + 40]], np.int64)
    c["sz"] = np.array([[100, 100]], np.int64)
    c["cells"] = np.array([[1, 2]], np.int64)
    c["npl"] = np.array([2], np.int64)
    return c
