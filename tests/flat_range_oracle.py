"""Oracle of tpq_flat_range_count / tpq_flat_range_fill (test infrastructure; semantics: include/torchpq_amd.h): the
values of tests/flat_oracle.py (+ 0.f: -0.0 is returned as +0.0), and as hits the live slots whose value is >= the
query's threshold -- a NaN on either side fails the compare -- in address order."""
import numpy as np

import flat_oracle as florc


def values(vectors, query, distance="euclidean"):
    """[nq, n] f32: tpq_flat_topk's values as the range search returns them"""
    fn = florc.values_d1 if vectors.shape[0] == 1 else florc.values
    with np.errstate(all="ignore"):
        return (fn(np.asarray(vectors, np.float32), np.asarray(query, np.float32), distance)
                + np.float32(0)).astype(np.float32)


def range_hits(vals, threshold, address2id=None):
    """value rows [nq, n], threshold a float or f32 [nq] -> (lims i64 [nq + 1], values f32 [total], address i64
    [total], ids i64 [total] or None).  `vals` is not changed: several thresholds may be applied to one array."""
    nq, n = vals.shape
    threshold = np.broadcast_to(np.asarray(threshold, np.float32), (nq,))
    live = np.ones(n, bool) if address2id is None else (np.asarray(address2id) >= 0)
    lims, v, a = np.zeros(nq + 1, np.int64), [np.zeros(0, np.float32)], [np.zeros(0, np.int64)]
    for q in range(nq):
        with np.errstate(invalid="ignore"):
            addr = np.nonzero(live & (vals[q] >= threshold[q]))[0]     # False for a NaN on either side
        v.append(vals[q, addr])
        a.append(addr.astype(np.int64))
        lims[q + 1] = lims[q] + len(addr)
    v, a = np.concatenate(v).astype(np.float32), np.concatenate(a)
    return lims, v, a, (None if address2id is None else np.asarray(address2id, np.int64)[a])


def range_search(vectors, query, threshold, address2id=None, distance="euclidean"):
    return range_hits(values(vectors, query, distance), threshold, address2id)


def sort_segments(lims, values, address, *more):
    """each query's segment by (value descending, address ascending): what range_search(sort=True) returns"""
    order = np.concatenate([lo + np.lexsort((address[lo:hi], -values[lo:hi].astype(np.float64)))
                            for lo, hi in zip(lims[:-1], lims[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    return tuple(t[order] for t in (values, address, *more))


def integer_problem(seed=11, d=40, n=700, nq=11, tomb=80):
    """components in -8 ... 8, d <= 40: every product, partial sum and norm is an integer below 2^24, so fp32 is exact
    whatever the order of summation -- this oracle, float64 brute force and the kernels of both indexes must agree to
    the bit.  A run of equal vectors gives exact ties.  -> (vectors [d, n], queries [d, nq], address2id [n])"""
    assert d <= 40
    rng = np.random.default_rng(seed)
    y = rng.integers(-8, 9, (d, n)).astype(np.float32)
    x = rng.integers(-8, 9, (d, nq)).astype(np.float32)
    y[:, 100:130] = y[:, 40:41]
    a2id = np.arange(n, dtype=np.int64) * 3 + 1
    a2id[rng.choice(n, tomb, replace=False)] = -1
    return y, x, a2id


def exact_values(vectors, query, distance):
    """float64 brute force [nq, n]"""
    y64, x64 = vectors.astype(np.float64), query.astype(np.float64)
    if distance == "euclidean":
        return -((x64.T[:, None, :] - y64.T[None, :, :]) ** 2).sum(-1)
    return x64.T @ y64
