"""Oracle of tpq_flat_topk (test infrastructure): the values of include/torchpq_amd.h through the C oracle's fmaf
chains, and the top-k by (value descending, address ascending) over the live slots whose value is not NaN."""
import numpy as np

from oracle import c_oracle


def values(vectors, query, distance="euclidean"):
    """[nq, n] f32: dot, |x|^2, |y|^2 as ascending-dimension fmaf chains from 0.f; v = (2 dot - |x|^2) - |y|^2 for
    "euclidean", dot otherwise.  c_oracle.adc_lut on [1, d, 256] blocks of the stored vectors, zero-padded, is
    exactly that, for both metrics."""
    vectors = np.ascontiguousarray(vectors, np.float32)
    query = np.ascontiguousarray(query, np.float32)
    d, n = vectors.shape
    nq = query.shape[1]
    out = np.empty((nq, max(n, 0)), np.float32)
    kind = "euclidean" if distance == "euclidean" else "inner"
    for c0 in range(0, n, 256):
        w = min(256, n - c0)
        block = np.zeros((1, d, 256), np.float32)
        block[0, :, :w] = vectors[:, c0:c0 + w]
        with np.errstate(all="ignore"):
            out[:, c0:c0 + w] = c_oracle.adc_lut(query, block, kind, n_threads=4)[0][:, :w]   # (small blocks: few threads)
    return out


def values_d1(vectors, query, distance="euclidean"):
    """d == 1: one rounding per operation in plain NumPy is the same arithmetic (fmaf(x, y, 0.f) = fl(x y))"""
    assert vectors.shape[0] == 1 and query.shape[0] == 1
    y = np.ascontiguousarray(vectors[0], np.float32)
    x = np.ascontiguousarray(query[0], np.float32)
    with np.errstate(all="ignore"):
        dot = x[:, None] * y[None, :]
        if distance != "euclidean":
            return dot
        v = np.float32(2.0) * dot
        v -= (x * x)[:, None]
        v -= (y * y)[None, :]
    return v


def topk(vals, k, address2id=None):
    """(values [nq, k], address [nq, k], ids [nq, k] or None) of value rows [nq, n]; pads (-inf, -1, -1)"""
    nq, n = vals.shape
    out_v = np.full((nq, k), -np.inf, np.float32)
    out_a = np.full((nq, k), -1, np.int64)
    live = np.ones(n, bool) if address2id is None else (np.asarray(address2id) >= 0)
    for q in range(nq):
        row = vals[q]
        ok = live & ~np.isnan(row)
        if ok.sum() > 4 * k:   # (only rows at or above the k-th largest value can enter)
            kth = np.partition(row[ok], -k)[-k]
            ok &= row >= kth
        addr = np.nonzero(ok)[0]
        order = np.lexsort((addr, -row[addr].astype(np.float64)))[:k]
        out_v[q, :len(order)] = row[addr[order]]
        out_a[q, :len(order)] = addr[order]
    ids = None
    if address2id is not None:
        ids = np.where(out_a >= 0, np.asarray(address2id)[np.maximum(out_a, 0)], -1).astype(np.int64)
    return out_v, out_a, ids


def search(vectors, query, k, address2id=None, distance="euclidean"):
    return topk(values(vectors, query, distance), k, address2id)
