"""Helpers shared between test modules: the k-means fit cases, and the IVFPQRIndex re-rank cases and checks."""
import numpy as np
import torch

# shared by the k-means fit tests: name -> (init key, n_redo, max_iter, tol key or value, seed key)
CASES = {
    "1": ("init", 1, 1, 0.0, None),
    "3": ("init", 1, 3, 0.0, None),
    "tol": ("init", 1, 12, "tol_exit", None),
    "redo": ("init", 2, 3, 0.0, "redo_seed"),
    "redo_b": ("bad_init", 2, 3, 0.0, "redo_b_seed"),
}

# ---- shared by the IVFPQRIndex GPU tests (test_gpu_ivfpqr.py, test_gpu_ivfpqr_edges.py) ----------------
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _case(seed, m, m_r, d, cap, nq, k1, distance, scale=None):
    """a random re-rank problem; `scale` (codebooks and query, for long vectors) multiplies after generation, so
    a case without it is what it always was"""
    rng = np.random.default_rng(seed)
    storage = rng.integers(0, 256, ((m + m_r) // 4, cap, 4), dtype=np.uint8)
    cb = rng.standard_normal((m, d // m, 256)).astype(np.float32)
    cb_r = (0.3 * rng.standard_normal((m_r, d // m_r, 256))).astype(np.float32)
    query = rng.standard_normal((d, nq)).astype(np.float32)
    if distance == "cosine":
        query = (query / np.linalg.norm(query, axis=0, keepdims=True)).astype(np.float32)
    cand = np.argsort(rng.random((nq, cap)), axis=1)[:, :k1].astype(np.int64)   # distinct per row
    # rows with fewer than k real candidates (holes anywhere in the row), and rows with none
    short = rng.random(nq) < 0.3
    cand[short[:, None] & (rng.random((nq, k1)) < 0.7)] = -1
    cand[rng.random(nq) < 0.1] = -1
    if nq >= 3:
        cand[1] = -1
    a2i = rng.permutation(cap).astype(np.int64) * 3 + 1
    if scale is not None:
        cb, cb_r = (cb * np.float32(scale)).astype(np.float32), (cb_r * np.float32(scale)).astype(np.float32)
        if distance != "cosine":
            query = (query * np.float32(scale)).astype(np.float32)
    return storage, cb, cb_r, query, cand, a2i


def _run_and_compare(storage, cb, cb_r, query, cand, a2i, k, use_residual, distance, m):
    import ivfpqr_oracle as rorc
    from torchpq_amd.kernels import IVFPQRerankHip
    v, a, i = IVFPQRerankHip()(T(storage), m, T(cb) if use_residual else None, T(cb_r), T(query), T(cand), k,
                               use_residual=use_residual, distance=distance, address2id=T(a2i))
    ev, ea, ei = rorc.rerank(storage, cb, cb_r, query, cand, k, use_residual, distance, a2i)
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(N(i), ei)
    return N(v), N(a), N(i)


def _clustered(seed, d, n, nq, n_centers=40, spread=4.0):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((d, n_centers)) * spread
    base = (centers[:, rng.integers(0, n_centers, n)] + rng.standard_normal((d, n))).astype(np.float32)
    queries = (base[:, rng.choice(n, nq, replace=False)] + 0.3 * rng.standard_normal((d, nq))).astype(np.float32)
    return base, queries


def _normalize(idx, x):
    from torchpq_amd import util
    return util.normalize(x, dim=0)


def _expected_search(idx, x, k, rows=None):
    """tests/ivfpqr_oracle.search driven by the index's own coarse step (the pattern of test_gpu_index.py);
    `rows`: only these queries of the batch (the coarse step still sees the whole batch)"""
    import ivfpqr_oracle as rorc
    x = np.asarray(x, dtype=np.float32)
    if idx.distance == "cosine":
        x = N(_normalize(idx, T(x)))
    _, cells, npl = idx.probe(T(x))
    cells, npl = N(cells), N(npl)
    if rows is not None:
        x, cells, npl = np.ascontiguousarray(x[:, rows]), np.ascontiguousarray(cells[rows]), npl[rows]
    return rorc.search(x, N(idx.pq_codec.codebook), N(idx.pq_rerank_codec.codebook), N(idx._storage),
                       N(idx._is_empty), N(idx._cell_start), N(idx._cell_size), N(idx._address2id), cells,
                       npl, k, idx.rerank_factor, idx.use_residual, idx.distance)


def _check_search(idx, queries, k):
    v, i, a = idx.search(T(queries), k=k, return_address=True)
    ev, ei, ea = _expected_search(idx, queries, k)
    assert v.shape == (queries.shape[1], k) and v.dtype == torch.float32 and i.dtype == torch.int64
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(N(i), ei)
    v2, i2 = idx.search(T(queries), k=k)
    assert torch.equal(v2, v) and torch.equal(i2, i)
    return N(v), N(i)
