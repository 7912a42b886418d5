"""GPU: the re-rank kernel (tpq_ivfpqr_rerank) and IVFPQRIndex against tests/ivfpqr_oracle.py -- values
bit-equal, addresses and ids equal."""
import io

import numpy as np
import pytest
import torch

import ivfpqr_oracle as rorc
from tests_support import (DEV, N, T, _case, _check_search, _clustered, _expected_search, _normalize,
                           _run_and_compare)

pytestmark = pytest.mark.gpu

# (m, m_r, d): sub-vector lengths (ds, ds_r) = (2, 2), (4, 2), (1, 1), (4, 8), and (6, 2) with d not a multiple of 16
SHAPES = [(8, 8, 16), (16, 32, 64), (64, 64, 64), (32, 16, 128), (4, 12, 24)]
K1_K = [(1, 1), (7, 3), (64, 64), (200, 100), (1024, 512), (1024, 1024)]


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
@pytest.mark.parametrize("use_residual", [True, False])
@pytest.mark.parametrize("m,m_r,d", SHAPES)
def test_rerank_kernel_matches_oracle(m, m_r, d, use_residual, distance):
    for k1, k in K1_K:
        for nq in (1, 3, 1000):
            cap = max(1500, k1 + 100)
            case = _case(1000 * k1 + nq + m, m, m_r, d, cap, nq, k1, distance)
            _run_and_compare(*case, k, use_residual, distance, m)


def test_rerank_kernel_exact_ties_are_ordered_by_address():
    m, m_r, d, cap, nq, k1 = 8, 8, 16, 4000, 5, 200
    storage, cb, cb_r, query, cand, a2i = _case(11, m, m_r, d, cap, nq, k1, "euclidean")
    cand = np.argsort(np.random.default_rng(12).random((nq, cap)), axis=1)[:, :k1].astype(np.int64)
    for q in range(nq):                      # every candidate shares its code pair with three others
        for g in range(0, k1, 4):
            storage[:, cand[q, g + 1:g + 4]] = storage[:, cand[q, g]][:, None]
    for use_residual in (True, False):
        _run_and_compare(storage, cb, cb_r, query, cand, a2i, 100, use_residual, "euclidean", m)
    ev, ea, _ = rorc.rerank(storage, cb, cb_r, query, cand, 100, True, "euclidean", a2i)
    tied = ev[:, 1:] == ev[:, :-1]
    assert tied.sum() > nq * 50 and np.all(ea[:, 1:][tied] > ea[:, :-1][tied])
    # the same address twice in a row of candidates: both are kept, next to each other
    cand[:, 1] = cand[:, 0]
    _run_and_compare(storage, cb, cb_r, query, cand, a2i, 100, True, "euclidean", m)


def test_rerank_kernel_addresses_beyond_2_pow_24():
    m, m_r, d, nq, k1 = 8, 8, 32, 3, 64
    cap = (1 << 24) + 50000
    rng = np.random.default_rng(5)
    touched = np.concatenate([rng.choice(1 << 24, 200, replace=False),
                              (1 << 24) + rng.choice(50000, 800, replace=False)]).astype(np.int64)
    storage = np.zeros(((m + m_r) // 4, cap, 4), np.uint8)
    storage[:, touched] = rng.integers(0, 256, (storage.shape[0], touched.size, 4), dtype=np.uint8)
    _, cb, cb_r, query, _, _ = _case(6, m, m_r, d, 8, nq, 1, "euclidean")
    cand = np.stack([rng.choice(touched, k1, replace=False) for _ in range(nq)])
    cand[2, ::3] = cap            # out of range: no candidate
    a2i = np.arange(cap, dtype=np.int64)[::-1].copy()
    assert (cand > (1 << 24)).sum() > nq * k1 // 2
    _run_and_compare(storage, cb, cb_r, query, cand, a2i, 32, True, "euclidean", m)


def test_rerank_kernel_declines_what_it_does_not_support():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFPQRerankHip
    storage, cb, cb_r, query, cand, a2i = _case(1, 8, 8, 16, 100, 2, 4, "euclidean")
    with pytest.raises(AssertionError):
        IVFPQRerankHip()(T(storage), 8, T(cb), T(cb_r), T(query), T(cand), 5)     # k > k1
    with pytest.raises(TorchPQAmdError):
        IVFPQRerankHip()(torch.from_numpy(storage), 8, T(cb), T(cb_r), T(query), T(cand), 2)   # a CPU tensor


def test_rerank_under_a_captured_graph():
    """replay equals eager (the process keeps its default number of hardware queues)"""
    from torchpq_amd.kernels import IVFPQRerankHip
    m, m_r, d = 16, 32, 64
    storage, cb, cb_r, query, cand, a2i = _case(21, m, m_r, d, 3000, 40, 200, "euclidean")
    args = (T(storage), m, T(cb), T(cb_r), T(query), T(cand), 100)
    op = IVFPQRerankHip()
    a2i_dev = T(a2i)
    eager = op(*args, address2id=a2i_dev)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op(*args, address2id=a2i_dev)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(*args, address2id=a2i_dev)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


# ---- the index -----------------------------------------------------------------------------------------
def _build(distance="euclidean", use_residual=True, d=32, m=8, m_r=8, n_cells=128, n=6000, seed=0, **kw):
    from torchpq_amd.index import IVFPQRIndex
    base, queries = _clustered(seed, d, n, 60)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFPQRIndex(d, n_subvectors=m, n_subvectors_rerank=m_r, n_cells=n_cells, use_residual=use_residual,
                      initial_size=16, distance=distance, device=DEV, **kw)
    idx.train(T(base))
    ids = torch.arange(n, device=DEV) * 2 + 5
    idx.add(T(base[:, :n // 3]), ids=ids[:n // 3])
    idx.add(T(base[:, n // 3:]), ids=ids[n // 3:])
    return idx, base, queries, ids


def test_constructor_contract_and_layout():
    from torchpq_amd.codec import PQCodec, VQCodec
    from torchpq_amd.index import IVFPQRIndex
    idx = IVFPQRIndex(64, n_subvectors=16, n_subvectors_rerank=32, n_cells=8, initial_size=4, device=DEV)
    assert (idx.d_vector, idx.n_subvectors, idx.n_subvectors_rerank, idx.n_cells) == (64, 16, 32, 8)
    assert idx.use_residual is True and idx.distance == "euclidean" and idx.rerank_factor == 2
    assert idx.code_size == 48 and idx.contiguous_size == 4
    assert tuple(idx._storage.shape) == (12, 32, 4) and idx._storage.dtype == torch.uint8
    assert isinstance(idx.vq_codec, VQCodec) and isinstance(idx.pq_codec, PQCodec)
    assert isinstance(idx.pq_rerank_codec, PQCodec) and idx.pq_rerank_codec.n_subvectors == 32
    assert idx.pq_use_residual is False
    idx.set_pq_rerank_codec_max_iter(3)
    assert idx.pq_rerank_codec.kmeans.max_iter == 3 and idx.pq_codec.kmeans.max_iter == 25
    idx.rerank_factor = 4
    with pytest.raises(AssertionError):
        idx.rerank_factor = 0
    with pytest.raises(AssertionError, match="not trained"):
        idx.search(torch.zeros(64, 2, device=DEV), k=4)
    with pytest.raises(AssertionError, match="rerank_factor"):
        idx.search(torch.zeros(64, 2, device=DEV), k=257)
    with pytest.raises(AssertionError):
        idx.search(torch.zeros(64, 2, device=DEV), k=0)


@pytest.mark.parametrize("distance,use_residual", [("euclidean", True), ("cosine", True), ("euclidean", False),
                                                   ("cosine", False)])
def test_index_end_to_end_against_oracle(distance, use_residual):
    idx, base, queries, ids = _build(distance, use_residual)
    n = base.shape[1]
    assert idx.n_items == n and tuple(idx._storage.shape[::2]) == (4, 4)
    # stored codes == encode(x) (both codes), in the cell the coarse quantizer assigns
    adr = idx.get_address_by_id(ids)
    xb = T(base)
    codes = idx.encode(xb)
    assert codes.shape == (16, n) and codes.dtype == torch.uint8
    assert torch.equal(idx.get_data_by_address(adr), codes)
    xn = _normalize(idx, xb) if distance == "cosine" else xb
    assert torch.equal(idx.get_cell_by_address(adr), idx.vq_codec.encode(xn.contiguous()))
    first = idx.pq_codec.decode(codes[:8])
    second = idx.pq_rerank_codec.decode(codes[8:])
    assert torch.equal(idx.decode(codes), second + first if use_residual else second)
    if use_residual:  # the second code shrinks the reconstruction error (legacy/IVFPQR.py:298-313)
        assert float(((xn - idx.decode(codes)) ** 2).sum()) < 0.5 * float(((xn - first) ** 2).sum())
    for smart in (False, True):
        for packed in (False, True):
            for n_probe in (1, 80):
                idx.use_smart_probing, idx.use_packed_layout, idx.n_probe = smart, packed, n_probe
                for k, factor in ((1, 1), (10, 2), (100, 4)):
                    idx.rerank_factor = factor
                    _check_search(idx, queries, k)
    idx.rerank_factor, idx.n_probe = 2, 16
    want = _check_search(idx, queries, 10)
    idx.max_query_batch = 7
    split = idx.search(T(queries), k=10)
    assert np.array_equal(N(split[0]), want[0]) and np.array_equal(N(split[1]), want[1])
    idx.max_query_batch = 32768
    # remove: the best hits of the first queries disappear from every answer
    gone = torch.from_numpy(np.unique(want[1][:20, :3].ravel())).to(DEV)
    gone = gone[gone >= 0]
    idx.remove(ids=gone)
    assert idx.n_items == n - gone.numel()
    _, i_after = _check_search(idx, queries, 10)
    assert not np.isin(i_after, N(gone)).any()
    # and a later add lands behind the survivors and is found
    idx.add(T(base[:, :50]), ids=torch.arange(50, device=DEV) + 10 ** 6)
    _check_search(idx, queries, 10)


def test_index_with_nothing_added():
    from torchpq_amd.index import IVFPQRIndex
    base, queries = _clustered(3, 32, 3000, 9)
    np.random.seed(3)
    idx = IVFPQRIndex(32, n_subvectors=8, n_subvectors_rerank=16, n_cells=16, initial_size=8, device=DEV)
    idx.train(T(base))
    idx.n_probe = 4
    v, i = idx.search(T(queries), k=5)
    assert torch.all(torch.isneginf(v)) and torch.all(i == -1)
    _check_search(idx, queries, 5)


def test_state_dict_has_the_reference_keys_and_round_trips():
    from torchpq_amd.index import IVFPQRIndex
    idx, base, queries, ids = _build(m_r=16)
    idx.n_probe = 8
    want = _check_search(idx, queries, 10)
    buf = io.BytesIO()
    torch.save(idx.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    assert set(sd) == {"_address2id", "_storage", "_cell_start", "_cell_size", "_cell_capacity", "_is_empty",
                       "vq_codec._is_trained", "vq_codec.kmeans.centroids",
                       "pq_codec._is_trained", "pq_codec.kmeans.centroids",
                       "pq_rerank_codec._is_trained", "pq_rerank_codec.kmeans.centroids"}
    cap = sd["_address2id"].shape[0]
    assert tuple(sd["_storage"].shape) == (6, cap, 4) and sd["_storage"].dtype == torch.uint8
    assert tuple(sd["vq_codec.kmeans.centroids"].shape) == (32, 128)
    assert tuple(sd["pq_codec.kmeans.centroids"].shape) == (8, 4, 256)
    assert tuple(sd["pq_rerank_codec.kmeans.centroids"].shape) == (16, 2, 256)
    fresh = IVFPQRIndex(32, n_subvectors=8, n_subvectors_rerank=16, n_cells=128, device=DEV)
    fresh.load_state_dict(sd)
    fresh.n_probe = 8
    assert fresh.n_items == idx.n_items and fresh.max_id == idx.max_id
    got = _check_search(fresh, queries, 10)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_first_stage_is_the_unchanged_ivfpq_search():
    """rerank_factor = 1 re-orders the first stage's k: the id SET per query is that of an IVFPQIndex with the
    same coarse / PQ state and the same vectors"""
    from torchpq_amd.index import IVFPQIndex
    idx, base, queries, ids = _build()
    plain = IVFPQIndex(32, n_subvectors=8, n_cells=128, initial_size=16, device=DEV)
    plain.vq_codec.load_state_dict(idx.vq_codec.state_dict())
    plain.pq_codec.load_state_dict(idx.pq_codec.state_dict())
    n = base.shape[1]
    plain.add(T(base[:, :n // 3]), ids=ids[:n // 3])
    plain.add(T(base[:, n // 3:]), ids=ids[n // 3:])
    assert torch.equal(plain._storage, idx._storage[:2])
    idx.rerank_factor = 1
    for packed in (False, True):
        for n_probe, k in ((1, 5), (16, 10), (80, 100)):
            for index in (idx, plain):
                index.n_probe, index.use_packed_layout = n_probe, packed
            _, mine = idx.search(T(queries), k=k)
            _, theirs = plain.search(T(queries), k=k)
            assert np.array_equal(np.sort(N(mine), axis=1), np.sort(N(theirs), axis=1))


def test_rerank_buys_recall():
    """recall@10 against exact search on a seeded clustered set, n_probe = n_cells (the coarse step does not
    cap it): rerank_factor = 4 beats the first stage alone (rerank_factor = 1) on the same trained index, and
    equals what the oracle search reaches on the same index state."""
    from torchpq_amd.index import FlatIndex, IVFPQRIndex
    d, n, nq, k = 32, 20000, 200, 10
    base, queries = _clustered(0, d, n, nq, n_centers=50)
    np.random.seed(0)
    idx = IVFPQRIndex(d, n_subvectors=8, n_subvectors_rerank=8, n_cells=32, initial_size=256, device=DEV)
    idx.train(T(base))
    idx.add(T(base))
    idx.n_probe = 32
    idx.use_smart_probing = False
    flat = FlatIndex(d, device=DEV)
    flat.add(T(base))
    _, truth = flat.search(T(queries), k=k)
    truth = N(truth)

    def recall(found):
        return float(np.mean([len(np.intersect1d(found[q], truth[q])) / k for q in range(nq)]))

    idx.rerank_factor = 1
    first = recall(N(idx.search(T(queries), k=k)[1]))
    idx.rerank_factor = 4
    reranked = recall(N(idx.search(T(queries), k=k)[1]))
    oracle = recall(_expected_search(idx, queries, k)[1])
    print(f"recall@10: first stage {first:.4f}, rerank_factor=4 {reranked:.4f}, oracle {oracle:.4f}")
    assert reranked > first and reranked >= oracle, \
        f"recall@10 first stage {first:.4f}, re-ranked {reranked:.4f}, oracle search {oracle:.4f}"
