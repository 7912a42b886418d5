"""The list-scan cases of the residual IVFPQ4Index tests, shared by test_ivfpq4_residual_cpu.py (what the inputs are)
and test_gpu_ivfpq4_residual.py (the kernel on them): the cases of tests/ivfpq4_cases.py -- the same cells of 0, 1, 63,
64, 65, 300, 17 and 128 slots, junk in the free slots, duplicated codes, tombstones, one duplicated probe, n_probe_list
below, at and beyond max_nprobe -- plus the probed cells themselves and one N(0,1) centroid per cell."""
import numpy as np

import ivfpq4_cases as plain
import ivfpq4_residual_oracle as rorc
from ivfpq4_oracle import probed_slots, unpack

CELL_SIZES = plain.CELL_SIZES

# The case whose summation order decides places: ivfpq4_cases.OFFSET_CASE's inputs (seed 4242, m = 64, nq = 3,
# n_probe = 8, k = 10; codebook -2^20 + N(0,1), ds = 1, query all ones) with every centroid component -2^20.
# Seed 4242 as it stands: test_ivfpq4_residual_cpu checks that a pairwise sum picks another top-k set there.
OFFSET_SEED = plain.OFFSET_CASE[0]


def case(seed, m, ds, nq, n_probe, tomb=25, dup=True, sizes=CELL_SIZES, offset=0.0):
    """ivfpq4_cases.case(...) plus `cells` i64 [nq, n_probe] and `centroids` f32 [n_cells, d].  The cells are
    recovered from the case's own `cs` (every cell has its own start), so the plain case is used as it is."""
    c = plain.case(seed, m, ds, nq, n_probe, tomb=tomb, dup=dup, sizes=sizes, offset=offset)
    rng = np.random.default_rng(seed)
    caps = np.array(sizes, np.int64) + rng.integers(1, 9, len(sizes))     # the builder's first draw
    start = (np.cumsum(caps) - caps).astype(np.int64)
    cells = np.searchsorted(start, c["cs"]).astype(np.int64)
    assert np.array_equal(start[cells], c["cs"]) and np.array_equal(np.array(sizes, np.int64)[cells], c["sz"])
    centroids = np.random.default_rng(seed + 1).standard_normal((len(sizes), m * ds)).astype(np.float32)
    return dict(c, cells=cells, centroids=centroids)


def offset_case(seed=OFFSET_SEED):
    _, m, nq, n_probe, k = plain.OFFSET_CASE
    c = case(seed, m, 1, nq, n_probe, offset=-float(2 ** 20))
    c["centroids"][:] = -float(2 ** 20)
    return c, k


def pairwise_topk_sets(c, k, distance):
    """per query, the address set of the top-k when the m table entries are summed PAIRWISE in fp32 (a balanced tree)
    instead of the specification's ascending-j chain -- ivfpq4_cases.pairwise_topk_sets on the per-probe tables"""
    codes = unpack(c["storage"])
    table = rorc.lut(c["query"], c["codebook"], c["centroids"], c["cells"], distance)
    m = codes.shape[0]
    out = []
    for q in range(c["query"].shape[1]):
        p, s = rorc.probe_slots(c["cs"][q], c["sz"][q], c["npl"][q], codes.shape[1])
        live = c["is_empty"][s] == 0
        p, s = p[live], s[live]
        t = table[q][p[:, None], np.arange(m)[None, :], codes[:, s].T].astype(np.float32)   # [n, m]
        while t.shape[1] > 1:
            t = (t[:, 0::2] + t[:, 1::2]).astype(np.float32)                                # (m is a power of two here)
        order = np.lexsort((s, -t[:, 0].astype(np.float64)))[:k]
        out.append(set(s[order].tolist()))
    return out


def scan(c, k, distance, with_empty=True):
    """the oracle on a case"""
    return rorc.scan_topk(c["storage"], c["query"], c["codebook"], c["centroids"], c["cells"],
                          c["is_empty"] if with_empty else None, c["cs"], c["sz"], c["npl"], k,
                          "euclidean" if distance == "euclidean" else "inner")
