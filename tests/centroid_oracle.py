"""Plain numpy reference for the k-means centroid update (tpq_compute_centroids, csrc/centroid_update.hip; the Lloyd
step's update_kernel, csrc/lloyd.hip): float64 means, a per-element error bound, seeded input families and an fp32
emulation of each route's summation.  A helper module (no tests, no fixtures); tests/test_centroid_oracle_cpu.py shows
without a GPU that the bound and the families are neither too tight nor blind.

Layout as the kernels have it: data [l, d, n] float32, labels [l, n] int64, centroids [l, d, k] float32.

THE BOUND (bound()).  A centroid element is fl(S^ / c): S^ the fp32 sum, in some order, of the cluster's T addends
(T = c on the scalar routes; T = 3 c on the matrix route, whose bf16 pieces satisfy |h| + |m| + |lo| <= 1.005 |x|) and
of the P per-block partial sums that global atomics combine; c, a count, is exact.  With u = 2^-24, A = sum |x_i| over
the cluster and standard summation analysis |S^ - S| <= (T + P) u A to first order, the division adds u |S / c|:

    |centroid - mean64| <= 2 * ((T + P) u A / c) + 2 u |mean64|

The factor 2 covers the undocumented rounding inside a 16-term MFMA accumulation; it may be tightened by a derivation,
never loosened.  An empty cluster has bound 0: it must be exactly 0.

EXACT FAMILIES pin what a bound cannot: `singletons` (one point per cluster: the output is that point's value bit for
bit -- h + m + lo == x exactly and x / 1 == x; every other point carries an out-of-range label), `integers_wide` and
`integers_small` (every partial sum in any order is an integer below 2^24: the output is float32(S / c) bit for bit).
"""
import json
import os
import zlib

import numpy as np

U = 2.0 ** -24
KCC_DT = 16            # kCcDT, centroid_update.hip: dimensions per block of the LDS and global routes
KUM_P = 64             # kUmP: points per staged tile of the matrix route


def OUT_OF_RANGE(k):
    """the labels every accumulate kernel must skip"""
    return np.array([-1, k, k + 1, 2 ** 31, 2 ** 40, -2 ** 40], np.int64)


GENERAL = ("gauss", "offset", "mixed", "heavy")
LABELS = ("uniform", "one_first", "one_last", "one_mid", "skewed", "gaps_even", "gaps_odd")


# ---------------------------------------------------------------------------------------------------------------------
# launch rules of tpq_compute_centroids, restated
# ---------------------------------------------------------------------------------------------------------------------
def route(l, d, n, k):
    """'mfma' | 'lds' | 'global': the branches of tpq_compute_centroids (centroid_update.hip: `if (k <= 256 && d >= 32)`,
    then `if (!lds_fits)` with lds = (kCcDT + 1) * k * 4 bytes <= 160 KiB, i.e. k <= 2409)"""
    if k <= 256 and d >= 32:
        return "mfma"
    return "lds" if (KCC_DT + 1) * k * 4 <= 160 * 1024 else "global"


def partials(l, d, n, k):
    """P of bound(): per-block partial sums of one output element that global atomics combine.
    mfma   -- `chunks` of tpq_compute_centroids' matrix branch ("blocks per (sub-problem, dimension tile)": 4096 / CT /
              (l * dtiles) with CT = TPQ_UM_CT = 1, at most n_tiles / 64, at least 1): every block of a dimension tile
              adds its accumulator to sums[] once;
    lds    -- gridDim.x of centroid_accum_kernel: ceil(n / points), points = max(4096, ceil(n / chunks)) rounded up to
              256, chunks = max(1, 8192 / (l * dtiles)) ("aim for ~8 k blocks ... never fewer than 4096 points");
    global -- 0: centroid_accum_global_kernel sends every point straight to a global atomic (those are the T addends)."""
    r = route(l, d, n, k)
    if r == "mfma":
        dtiles = (d + 31) // 32
        chunks = 4096 // (l * dtiles)
        n_tiles = (n + KUM_P - 1) // KUM_P
        chunks = min(chunks, n_tiles // 64)
        return max(chunks, 1)
    if r == "lds":
        dtiles = (d + KCC_DT - 1) // KCC_DT
        chunks = max(1, 8192 // (l * dtiles))
        points = max(4096, (n + chunks - 1) // chunks)
        points = (points + 255) // 256 * 256
        return (n + points - 1) // points
    return 0


def addends_per_point(l, d, n, k):
    return 3 if route(l, d, n, k) == "mfma" else 1


# ---------------------------------------------------------------------------------------------------------------------
# float64 reference and bound
# ---------------------------------------------------------------------------------------------------------------------
def _sums64(values, labels, k):
    """sum of values[b, e, i] over labels[b, i] == j, in float64: [l, d, k]; counts [l, k]"""
    l, d, n = values.shape
    sums = np.zeros((l, d, k), np.float64)
    counts = np.zeros((l, k), np.int64)
    for b in range(l):
        ok = (labels[b] >= 0) & (labels[b] < k)
        lab = labels[b][ok]
        counts[b] = np.bincount(lab, minlength=k)
        vb = values[b][:, ok].astype(np.float64)
        for e in range(d):
            sums[b, e] = np.bincount(lab, weights=vb[e], minlength=k)
    return sums, counts


def mean64(data, labels, k):
    """float64 mean of every cluster over the labels in [0, k) only; an empty cluster gives 0"""
    sums, counts = _sums64(data, labels, k)
    c = counts[:, None, :]
    return np.where(c > 0, sums / np.maximum(c, 1), 0.0)


def bound(data, labels, k, addends_per_point, partials):
    """per element: 2 * ((T + P) u A / c) + 2 u |mean64| (module docstring); 0 for an empty cluster"""
    return mean_and_bound(data, labels, k, addends_per_point, partials)[1]


def mean_and_bound(data, labels, k, addends_per_point, partials):
    """(mean64, bound) in one pass over the data"""
    asum, counts = _sums64(np.abs(data.astype(np.float64)), labels, k)
    c = counts[:, None, :].astype(np.float64)
    t = c * addends_per_point
    m = mean64(data, labels, k)
    return m, np.where(c > 0, 2.0 * ((t + partials) * U * asum / np.maximum(c, 1)) + 2.0 * U * np.abs(m), 0.0)


def exact_mean32(data, labels, k):
    """float32(S / c) from exact integer sums (the integer families): correctly rounded fp32 division of two integers
    below 2^24, both exact in fp32"""
    sums, counts = _sums64(data, labels, k)
    assert np.array_equal(sums, np.rint(sums)) and np.abs(sums).max(initial=0) <= 2 ** 24 and counts.max() <= 2 ** 24
    c = counts[:, None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        q = sums.astype(np.float32) / np.broadcast_to(c, sums.shape).astype(np.float32)
    return np.where(c > 0, q, np.float32(0)).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# labels
# ---------------------------------------------------------------------------------------------------------------------
def make_labels(name, l, n, k, rng, out_of_range=False):
    """label families (LABELS); out_of_range: 5 % of the points (at least one when n > 1) get a label outside [0, k)"""
    if name == "uniform":
        lab = rng.integers(0, k, (l, n))
    elif name in ("one_first", "one_last", "one_mid"):
        lab = np.full((l, n), {"one_first": 0, "one_last": k - 1, "one_mid": k // 2}[name])
    elif name == "skewed":
        lab = np.where(rng.random((l, n)) < 0.9, int(rng.integers(0, k)), rng.integers(0, k, (l, n)))
    elif name in ("gaps_even", "gaps_odd"):     # even clusters only (the last is empty when k is even) / odd only
        first = 0 if (name == "gaps_even" or k == 1) else 1
        lab = first + 2 * rng.integers(0, (k - first + 1) // 2, (l, n))
    else:
        raise ValueError(name)
    lab = lab.astype(np.int64)
    assert lab.min() >= 0 and lab.max() < k
    if out_of_range and n > 1:
        bad = rng.random((l, n)) < 0.05
        bad[:, rng.integers(0, n)] = True
        lab = np.where(bad, rng.choice(OUT_OF_RANGE(k), (l, n)), lab)
    return lab


def cap_cluster_sizes(labels, k, cap, rng):
    """labels with every cluster cut down to `cap` points: the surplus points get out-of-range labels"""
    out = labels.copy()
    for b in range(labels.shape[0]):
        ok = np.flatnonzero((labels[b] >= 0) & (labels[b] < k))
        order = ok[np.argsort(labels[b][ok], kind="stable")]
        lab = labels[b][order]
        rank = np.arange(len(lab)) - np.searchsorted(lab, lab, side="left")
        surplus = order[rank >= cap]
        out[b, surplus] = rng.choice(OUT_OF_RANGE(k), len(surplus))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# data families
# ---------------------------------------------------------------------------------------------------------------------
def make_general(name, l, d, n, rng):
    if name == "gauss":
        x = rng.standard_normal((l, d, n))
    elif name == "offset":
        x = 1.0e4 + rng.standard_normal((l, d, n))
    elif name == "mixed":         # per-dimension scales 2^-20 .. 2^20
        x = rng.standard_normal((l, d, n)) * 2.0 ** rng.integers(-20, 21, (1, d, 1))
    elif name == "heavy":         # Student t, 1.5 degrees of freedom: a few elements dominate a sum
        x = rng.standard_t(1.5, (l, d, n))
    else:
        raise ValueError(name)
    x = x.astype(np.float32)
    assert np.isfinite(x).all()
    return x


def full_mantissa_values(shape, rng):
    """float32 with all 24 mantissa bits in use (the last one set), both signs, 2^-60 <= |x| < 2^60"""
    mant = (rng.integers(2 ** 22, 2 ** 23, shape, dtype=np.int64) * 2 + 1).astype(np.float64)   # odd, in [2^23, 2^24)
    x64 = np.ldexp(mant, rng.integers(-60, 60, shape) - 23) * rng.choice([-1.0, 1.0], shape)
    x = x64.astype(np.float32)
    assert np.array_equal(x.astype(np.float64), x64) and (x.view(np.uint32) & 1).all()    # no rounding, last bit set
    assert (np.abs(x) >= 2.0 ** -60).all() and (np.abs(x) < 2.0 ** 60).all()             # no zeros, no denormals
    return x


def make_singletons(l, d, n, k, rng):
    """(data, labels, expected): every label of [0, k) exactly once, everything else out of range; the expected
    centroid is the labelled point itself, bit for bit.  Needs n >= k."""
    assert n >= k, "singletons: one point per cluster needs n >= k"
    x = full_mantissa_values((l, d, n), rng)
    lab = rng.choice(OUT_OF_RANGE(k), (l, n))
    expected = np.zeros((l, d, k), np.float32)
    for b in range(l):
        where = rng.permutation(n)[:k]
        lab[b, where] = np.arange(k)
        expected[b] = x[b][:, where]
    for b in range(l):      # the precondition: every in-range label exactly once
        ok = (lab[b] >= 0) & (lab[b] < k)
        assert np.array_equal(np.sort(lab[b][ok]), np.arange(k))
    return x, lab.astype(np.int64), expected


def make_integers_wide(labels, l, d, n, k, rng):
    """(data, labels', expected): integers in [-2^20, 2^20), the given labels cut down to 16 points per cluster.
    Preconditions: max |x| * max c <= 2^24, and the same for the bf16 pieces (sum of |h| + |m| + |lo| per cluster):
    every partial sum, in any order, of values or of pieces, is then an integer of at most 2^24 -- exact."""
    x = rng.integers(-2 ** 20, 2 ** 20, (l, d, n)).astype(np.float32)
    lab = cap_cluster_sizes(labels, k, 16, rng)
    _, counts = _sums64(x, lab, k)
    assert counts.max() <= 16 and np.abs(x).max() * counts.max() <= 2 ** 24
    h, m, lo = split3_bf16(x)
    piece_sums, _ = _sums64(np.abs(h).astype(np.float64) + np.abs(m) + np.abs(lo), lab, k)
    assert piece_sums.max(initial=0) <= 2 ** 24
    return x, lab, exact_mean32(x, lab, k)


def make_integers_small(labels, l, d, n, k, rng):
    """(data, labels, expected): integers in [0, 256), any labels.  Precondition: 255 * max c <= 2^24 (the pieces of
    such a value are h = x, m = lo = 0 or all non-negative integers summing to x, so the same holds for them)"""
    x = rng.integers(0, 256, (l, d, n)).astype(np.float32)
    _, counts = _sums64(x, labels, k)
    assert 255 * counts.max() <= 2 ** 24
    return x, labels, exact_mean32(x, labels, k)


# ---------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the routes' summation
# ---------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float32 -> nearest bfloat16 (ties to even), as float32"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(np.float32)


def split3_bf16(x):
    """split3_bf16 of mfma_util.h: x == h + m + lo exactly"""
    x = np.asarray(x, np.float32)
    h = bf16_rne(x)
    r1 = (x - h).astype(np.float32)
    m = bf16_rne(r1)
    lo = bf16_rne((r1 - m).astype(np.float32))
    return h, m, lo


def emulate(data, labels, k, order="ascending", blocks=1, pieces=1, rng=None, drop_third=False, leak_out_of_range=False,
            count_per_dtile=1):
    """fp32 emulation of one route: every addition rounds to float32.
    order  -- 'ascending' | 'descending' | 'random': the order of the points within a block;
    blocks -- per-block partial sums (points dealt to the blocks in tiles of 64, round-robin, as the matrix route
              deals them; with blocks == 1 that is the whole range), combined in block order;
    pieces -- 1: the values themselves; 3: the matrix route -- per group of 16 points all h, then all m, then all lo.
    The last three switch on one WRONG behaviour each (the knock-outs of the CPU test): the third piece omitted, the
    first out-of-range point of every sub-problem added to cluster 0, counts taken count_per_dtile times."""
    l, d, n = data.shape
    rng = rng or np.random.default_rng(0)
    src = split3_bf16(data) if pieces == 3 else (np.asarray(data, np.float32),)
    if pieces == 3 and drop_third:
        src = src[:2]
    out = np.zeros((l, d, k), np.float32)
    for b in range(l):
        lab = labels[b].copy()
        if leak_out_of_range:
            bad = np.flatnonzero((lab < 0) | (lab >= k))
            if len(bad):
                lab[bad[0]] = 0
        idx = np.arange(n)
        tile = idx // KUM_P
        total = np.zeros((d, k), np.float32)
        cnt = np.zeros(k, np.int64)
        for blk in range(blocks):
            mine = idx[tile % blocks == blk]
            if order == "descending":
                mine = mine[::-1]
            elif order == "random":
                mine = rng.permutation(mine)
            mine = mine[(lab[mine] >= 0) & (lab[mine] < k)] if pieces == 1 else mine
            acc = np.zeros((d, k), np.float32)
            for g in range(0, len(mine), 16):
                group = mine[g:g + 16]
                for piece in src:
                    for i in group:
                        j = lab[i]
                        if 0 <= j < k:
                            acc[:, j] += piece[b, :, i]
            np.add.at(cnt, lab[mine][(lab[mine] >= 0) & (lab[mine] < k)], 1)
            total = (total + acc).astype(np.float32)
        cnt = cnt * count_per_dtile
        with np.errstate(invalid="ignore", divide="ignore"):
            q = total / cnt[None, :].astype(np.float32)
        out[b] = np.where(cnt[None, :] > 0, q, np.float32(0))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# shared by the GPU tests
# ---------------------------------------------------------------------------------------------------------------------
def seed(*key):
    return zlib.crc32(repr(key).encode())


def record(route, family, ratio):
    path = os.environ.get("TPQ_CENTROID_ERROR_JSON")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.setdefault("what", "largest |centroid - mean64| / bound over every element of every case of tests/"
                           "test_gpu_centroid_update.py and tests/test_gpu_lloyd_update.py, per route and data family "
                           "(MI355X); records, not bounds: above 1 is a kernel bug")
    cases = doc.setdefault("cases", {})
    key = f"{route}-{family}"
    cases[key] = {"error_over_bound": max(float(ratio), cases.get(key, {}).get("error_over_bound", 0.0))}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
