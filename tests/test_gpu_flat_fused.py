"""GPU: FlatIndex.use_fused_search -- the default route never reaches the fused kernel; the fused route against
tests/flat_oracle.py on the index's own state; the two routes agree; integer data equals float64 brute force."""
import numpy as np
import pytest
import torch

import flat_oracle as florc
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu


def _oracle(index, queries, k):
    """the oracle on the index's own storage and id map; for "cosine" queries and stored vectors divided by
    (norm + 1e-8), the normalisation of the default route (metric.cosine_similarity)"""
    q = queries
    storage = index._storage[:, :, 0]
    if index.distance == "cosine":
        q = N(T(queries) / (T(queries).norm(dim=-2, keepdim=True) + 1e-8))
        storage = storage / (storage.norm(dim=-2, keepdim=True) + 1e-8)
    return florc.search(N(storage), q, min(k, index.capacity), N(index._address2id), index.distance)


def _check(index, queries, k):
    v, i, a = index.search(T(queries), k=k, return_address=True)
    ev, ea, ei = _oracle(index, queries, k)
    assert np.array_equal(N(a), ea) and np.array_equal(N(i), ei)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    return N(v), N(i), N(a)


def _problem(seed=9, d=24, n=5000, nq=64, lengths=False):
    """`lengths`: the stored vectors (and the queries) get lengths spread over 0.2 ... 5, so that "cosine", "inner"
    and "euclidean" rank differently"""
    rng = np.random.default_rng(seed)
    base, queries = rng.standard_normal((d, n)).astype(np.float32), rng.standard_normal((d, nq)).astype(np.float32)
    if lengths:
        base *= np.exp(rng.uniform(np.log(0.2), np.log(5.0), n)).astype(np.float32)
        queries *= np.exp(rng.uniform(np.log(0.2), np.log(5.0), nq)).astype(np.float32)
    return base, queries


def test_default_route_never_reaches_the_fused_kernel(monkeypatch):
    from torchpq_amd.index import FlatIndex
    from torchpq_amd.kernels import FlatTopkHip

    def boom(*a, **kw):
        raise AssertionError("the fused kernel was called on the default route")
    monkeypatch.setattr(FlatTopkHip, "__call__", boom)
    base, queries = _problem(n=500)
    flat = FlatIndex(d_vector=24, initial_size=16, device=DEV)
    assert flat.use_fused_search is False
    flat.add(T(base))
    v, i = flat.search(T(queries), k=5)
    assert v.shape == (64, 5)
    flat.use_fused_search = True
    with pytest.raises(AssertionError, match="default route"):
        flat.search(T(queries), k=5)


@pytest.mark.parametrize("distance", ["euclidean", "cosine", "inner"])
def test_fused_route_equals_oracle_through_the_index_life_cycle(distance):
    from torchpq_amd.index import FlatIndex
    d, n, nq, k = 24, 5000, 64, 20
    base, queries = _problem(lengths=True)
    flat = FlatIndex(d_vector=d, initial_size=16, device=DEV, distance=distance)   # grows past initial_size
    flat.use_fused_search = True
    ids = torch.arange(n, device=DEV) * 2 + 5
    flat.add(T(base[:, :3000]), ids=ids[:3000])
    flat.add(T(base[:, 3000:4500]), ids=ids[3000:4500])
    assert flat.capacity > 16 and flat.n_items == 4500
    v, i, a = _check(flat, queries, k)
    v2, i2 = flat.search(T(queries), k=k)                         # return_address only adds the address
    assert np.array_equal(N(v2), v) and np.array_equal(N(i2), i)
    assert np.array_equal(i, np.where(a >= 0, a * 2 + 5, -1))
    # remove: the removed ids are never returned; add: the freed slots are used again
    gone = np.unique(i[:, 0])
    flat.remove(ids=T(gone))
    v3, i3, a3 = _check(flat, queries, k)
    assert not np.isin(i3, gone).any()
    new_ids, addr = flat.add(T(base[:, 4500:]), ids=ids[4500:], return_address=True)
    assert np.isin(np.unique(a[:, 0]), N(addr)).all()
    _check(flat, queries, k)
    # batches of max_query_batch give the same result as one batch
    q130 = np.concatenate([queries, queries[:, ::-1], queries[:, :2]], axis=1)
    whole = flat.search(T(q130), k=k)
    flat.max_query_batch = 50
    parts = flat.search(T(q130), k=k)
    assert all(torch.equal(x, y) for x, y in zip(whole, parts))
    del flat.max_query_batch
    assert flat.max_query_batch == 32768
    # state_dict round trip: the flag is not part of it
    assert not any("fused" in key or "max_query" in key for key in flat.state_dict())
    other = FlatIndex(d_vector=d, initial_size=flat.capacity, device=DEV, distance=distance)
    other.load_state_dict(flat.state_dict())
    assert other.use_fused_search is False
    other.use_fused_search = True
    assert all(torch.equal(x, y) for x, y in zip(other.search(T(queries), k=k), flat.search(T(queries), k=k)))


def test_k_above_the_items_width_and_pads_and_an_empty_index():
    from torchpq_amd.index import FlatIndex
    base, queries = _problem(n=40, nq=9)
    flat = FlatIndex(d_vector=24, initial_size=64, device=DEV)
    flat.use_fused_search = True
    v, i, a = flat.search(T(queries), k=5, return_address=True)    # capacity, no items: all pads
    assert v.shape == (9, 5) and torch.isneginf(v).all() and (i == -1).all() and (a == -1).all()
    flat.add(T(base))
    v, i, a = _check(flat, queries, 100)                           # width min(k, capacity) = 64, 40 candidates
    assert v.shape == (9, 64) and np.all(np.isfinite(v[:, :40]))
    assert np.all(np.isneginf(v[:, 40:])) and np.all(i[:, 40:] == -1) and np.all(a[:, 40:] == -1)
    flat.use_fused_search = False
    dv, di, da = flat.search(T(queries), k=100, return_address=True)
    assert dv.shape == (9, 64) and np.array_equal(N(di), i) and np.array_equal(N(da), a)


def test_the_two_routes_agree():
    """the data of test_flat_index_exact_search, with its tolerances against float64"""
    from torchpq_amd.index import FlatIndex
    d, n, nq, k = 24, 5000, 64, 20
    base, queries = _problem()
    flat = FlatIndex(d_vector=d, initial_size=16, device=DEV)
    ids = torch.arange(n, device=DEV) * 2 + 5
    flat.add(T(base[:, :3000]), ids=ids[:3000])
    flat.add(T(base[:, 3000:]), ids=ids[3000:])
    dv, di = flat.search(T(queries), k=k)
    flat.use_fused_search = True
    fv, fi = flat.search(T(queries), k=k)
    assert (N(fi) == N(di)).mean() > 0.999
    np.testing.assert_allclose(N(fv), N(dv), rtol=1e-4, atol=1e-4)
    d2 = -((queries.T[:, None, :] - base.T[None, :, :]) ** 2).sum(-1)
    order = np.argsort(-d2, axis=1, kind="stable")[:, :k]
    assert (N(fi) == N(ids)[order]).mean() > 0.999
    np.testing.assert_allclose(N(fv), np.take_along_axis(d2, order, 1), rtol=1e-4, atol=1e-4)


@pytest.mark.parametrize("distance", ["euclidean", "cosine", "inner"])
def test_the_two_routes_agree_on_vectors_of_unequal_length(distance):
    """stored vectors of lengths 0.2 ... 5: the three distances rank differently, and each route must rank as the
    other does -- "cosine" divides the stored vectors by their norms on both routes"""
    from torchpq_amd.index import FlatIndex
    d, n, nq, k = 24, 5000, 64, 20
    base, queries = _problem(seed=10, lengths=True)
    flat = FlatIndex(d_vector=d, initial_size=n, device=DEV, distance=distance)
    ids = torch.arange(n, device=DEV) * 3 + 1
    flat.add(T(base), ids=ids)
    flat.remove(ids=ids[::13])
    dv, di = flat.search(T(queries), k=k)
    flat.use_fused_search = True
    fv, fi = flat.search(T(queries), k=k)
    assert (N(fi) == N(di)).mean() > 0.999
    np.testing.assert_allclose(N(fv), N(dv), rtol=1e-4, atol=1e-4)
    # against float64, and the distances do differ on these data
    b64, q64 = base.astype(np.float64), queries.astype(np.float64)
    if distance == "euclidean":
        exact = -((q64.T[:, None, :] - b64.T[None, :, :]) ** 2).sum(-1)
    elif distance == "cosine":
        exact = (q64 / np.linalg.norm(q64, axis=0)).T @ (b64 / np.linalg.norm(b64, axis=0))
    else:
        exact = q64.T @ b64
    exact[:, ::13] = -np.inf
    order = np.argsort(-exact, axis=1, kind="stable")[:, :k]
    assert (N(fi) == N(ids)[order]).mean() > 0.999
    np.testing.assert_allclose(N(fv), np.take_along_axis(exact, order, 1), rtol=1e-4, atol=1e-4)
    l2 = -((q64.T[:, None, :] - b64.T[None, :, :]) ** 2).sum(-1)
    rival = l2 if distance == "inner" else q64.T @ b64           # another distance ranks these data differently
    rival[:, ::13] = -np.inf
    other = np.argsort(-rival, axis=1, kind="stable")[:, :k]
    assert (order == other).mean() < 0.5


def test_k_beyond_the_kernel_limit_raises_a_clear_error():
    from torchpq_amd.index import FlatIndex
    base, queries = _problem(n=1500, nq=3)
    flat = FlatIndex(d_vector=24, initial_size=1500, device=DEV)
    flat.add(T(base))
    v, i = flat.search(T(queries), k=1200)              # the default route takes any k
    assert v.shape == (3, 1200)
    flat.use_fused_search = True
    with pytest.raises(ValueError, match="1024"):
        flat.search(T(queries), k=1200)
    assert flat.search(T(queries), k=1024)[0].shape == (3, 1024)


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_integer_data_equals_float64_brute_force(distance):
    from torchpq_amd.index import FlatIndex
    rng = np.random.default_rng(6)
    d, n, nq, k = 16, 3000, 33, 50
    base = rng.integers(-3, 4, (d, n)).astype(np.float32)
    queries = rng.integers(-3, 4, (d, nq)).astype(np.float32)
    flat = FlatIndex(d_vector=d, device=DEV, distance=distance)
    flat.use_fused_search = True
    flat.add(T(base))
    flat.remove(ids=torch.arange(0, n, 11, device=DEV))
    v, i = flat.search(T(queries), k=k)
    b64, q64 = base.astype(np.float64), queries.astype(np.float64)
    slots = np.array([s for s in range(n) if s % 11])
    for q in range(nq):
        if distance == "euclidean":
            exact = -((q64[:, q:q + 1] - b64[:, slots]) ** 2).sum(0)
        else:
            exact = (q64[:, q:q + 1] * b64[:, slots]).sum(0)
        order = np.lexsort((slots, -exact))[:k]
        assert np.array_equal(N(i)[q], slots[order])
        assert np.array_equal(N(v)[q].astype(np.float64), exact[order])
