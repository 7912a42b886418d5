"""GPU: the IVFFlatIndex list scan (tpq_ivfflat_scan_topk) against tests/ivfflat_oracle.py -- values bit-equal,
addresses equal -- and the index end to end (placement, search, remove, expand, state_dict, reconstruct)."""
import numpy as np
import pytest
import torch

import ivfflat_oracle as forc
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu

# cells of 0, 1, 63, 64, 65 and about 300 slots (and two more), each with spare capacity behind it
CELL_SIZES = (0, 1, 63, 64, 65, 300, 17, 128)


def _case(seed, d, nq, n_probe, tomb=25, dup=True, sizes=CELL_SIZES, scale=1.0):
    rng = np.random.default_rng(seed)
    sizes = np.array(sizes, np.int64)
    n_cells = len(sizes)
    caps = sizes + rng.integers(1, 9, n_cells)
    start = (np.cumsum(caps) - caps).astype(np.int64)
    cap = int(caps.sum())
    vectors = (scale * rng.standard_normal((d, cap))).astype(np.float32)   # free slots hold finite junk
    query = (scale * rng.standard_normal((d, nq))).astype(np.float32)
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    live = np.flatnonzero(is_empty == 0)
    if dup:   # a third of the slots hold one of five vectors: ties everywhere, the k-th place included
        src = rng.choice(live, 5, replace=False)
        dst = rng.choice(live, len(live) // 3, replace=False)
        vectors[:, dst] = vectors[:, src[rng.integers(0, 5, len(dst))]]
        query[:, 0] = vectors[:, src[0]]
    if tomb:
        is_empty[rng.choice(live, tomb, replace=False)] = 1
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    if n_probe > 1 and nq > 1:
        cells[1, 1] = cells[1, 0]                       # one cell listed twice in a row: scanned once
    npl = rng.integers(0, n_probe + 3, nq).astype(np.int64)   # below, at and beyond max_nprobe
    npl[:max(1, nq // 2)] = n_probe
    return dict(vectors=vectors, query=query, is_empty=is_empty, cs=start[cells], sz=sizes[cells], npl=npl)


def _run(case, k, distance, n_split=None, op=None, with_empty=True):
    from torchpq_amd.kernels import IVFFlatTopkHip
    op = op or IVFFlatTopkHip()
    v, a = op(T(case["vectors"]), T(case["query"]), T(case["cs"]), T(case["sz"]), T(case["npl"]), k,
              is_empty=T(case["is_empty"]) if with_empty else None, distance=distance, n_split=n_split)
    return N(v), N(a), op


def _check(case, k, distance, n_split=None, with_empty=True):
    v, a, op = _run(case, k, distance, n_split, with_empty=with_empty)
    ev, ea = forc.scan_topk(case["vectors"], case["query"], case["is_empty"] if with_empty else None, case["cs"],
                            case["sz"], case["npl"], k, "euclidean" if distance == "euclidean" else "inner")
    assert v.shape == ev.shape and v.dtype == np.float32 and a.dtype == np.int64
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    return v, a, op


# (d, nq, n_probe, k, distance, n_split): every d, nq, n_probe and k of the list, both metrics, the wrapper's own
# choice of the split (None) and fixed ones; k = 1024 is above the live candidates of most rows
KERNEL_CASES = [
    (1, 3, 1, 1, "euclidean", None),
    (1, 1, 8, 1024, "inner", 3),
    (3, 1, 4, 10, "inner", None),
    (3, 1000, 8, 100, "euclidean", None),
    (24, 3, 8, 100, "euclidean", None),
    (24, 1000, 1, 10, "inner", None),
    (24, 3, 4, 1024, "euclidean", 1),
    (128, 1, 4, 100, "euclidean", None),
    (128, 1000, 4, 10, "euclidean", None),
    (128, 3, 8, 1024, "inner", None),
    (128, 3, 8, 200, "inner", 5),
    (128, 3, 4, 300, "euclidean", 2),
    (960, 3, 8, 10, "euclidean", None),
    (960, 1, 4, 1024, "inner", 7),
    (960, 3, 1, 1, "inner", None),
]


@pytest.mark.parametrize("d,nq,n_probe,k,distance,n_split", KERNEL_CASES)
def test_scan_against_the_oracle(d, nq, n_probe, k, distance, n_split):
    case = _case(1000 * d + nq + n_probe, d, nq, n_probe, scale=0.25 if d >= 960 else 1.0)
    v, a, op = _check(case, k, distance, n_split)
    # both launches run: the wrapper splits a small batch over several workgroups and leaves a large one whole
    if n_split is None:
        assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
    else:
        assert op.last_n_split == n_split
    live_probed = (a >= 0).sum(1)
    assert np.all(v[a < 0] == -np.inf) and np.all(v[:, 1:] <= v[:, :-1])
    if k == 1024:
        assert live_probed.min() < k        # k above the number of live candidates


def test_split_and_unsplit_agree_and_no_tombstone_mask():
    case = _case(77, 24, 5, 8, tomb=0)
    v1, a1, _ = _check(case, 100, "euclidean", 1, with_empty=False)
    v2, a2, _ = _check(case, 100, "euclidean", 6, with_empty=False)
    assert np.array_equal(a1, a2) and np.array_equal(v1.view(np.uint32), v2.view(np.uint32))


@pytest.mark.parametrize("n_split", [1, 4])
def test_equal_vectors_are_ordered_by_address(n_split):
    """every slot holds the same vector: all values tie, so the k best are the k lowest live addresses probed"""
    case = _case(5, 24, 3, 8, tomb=40, dup=False)
    case["vectors"][:] = case["vectors"][:, :1]
    for k in (1, 10, 100):
        v, a, _ = _check(case, k, "euclidean", n_split)
        for q in range(3):
            slots = forc.probed_slots(case["cs"][q], case["sz"][q], case["npl"][q], case["vectors"].shape[1])
            slots = np.sort(slots[case["is_empty"][slots] == 0])[:k]
            assert np.array_equal(a[q, :len(slots)], slots) and len(np.unique(v[q, :len(slots)])) <= 1


def test_addresses_beyond_2_pow_24():
    d, nq, k = 4, 3, 100
    cap = (1 << 24) + 50000
    rng = np.random.default_rng(5)
    # three cells of a few hundred slots: one below 2^24, one across it, one at the end of the storage
    start = np.array([1000, (1 << 24) - 150, cap - 260], np.int64)
    size = np.array([200, 300, 260], np.int64)
    vectors = np.zeros((d, cap), np.float32)
    is_empty = np.ones(cap, np.uint8)
    for st, sz in zip(start, size):
        vectors[:, st:st + sz] = rng.standard_normal((d, sz)).astype(np.float32)
        is_empty[st:st + sz] = 0
    is_empty[(1 << 24) + 7] = 1
    query = rng.standard_normal((d, nq)).astype(np.float32)
    cells = np.array([[0, 1, 2], [2, 1, 0], [1, 2, 0]])
    case = dict(vectors=vectors, query=query, is_empty=is_empty, cs=start[cells], sz=size[cells],
                npl=np.array([3, 3, 2], np.int64))
    v, a, _ = _check(case, k, "euclidean", 2)
    assert (a > (1 << 24)).sum() > nq * k // 3 and a.max() < cap


def test_a_nan_query_row_leaves_the_other_rows_alone():
    case = _case(9, 24, 6, 8)
    clean_v, clean_a, _ = _run(case, 10, "euclidean", 1)
    for n_split, bad in ((1, np.nan), (3, np.nan), (1, np.inf), (3, -np.inf)):
        dirty = dict(case, query=case["query"].copy())
        dirty["query"][5, 2] = bad
        v, a, _ = _run(dirty, 10, "euclidean", n_split)     # returns
        keep = [0, 1, 3, 4, 5]
        assert np.array_equal(a[keep], clean_a[keep])
        assert np.array_equal(v[keep].view(np.uint32), clean_v[keep].view(np.uint32))
        cap = case["vectors"].shape[1]
        assert np.all((a[2] >= -1) & (a[2] < cap))
        real = a[2][a[2] >= 0]
        assert len(np.unique(real)) == len(real)
        if np.isnan(bad):
            assert np.all(a[2] == -1) and np.all(np.isneginf(v[2]))   # a NaN value never enters


def test_wrapper_declines_what_it_does_not_support():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFFlatTopkHip
    case = _case(1, 8, 2, 2)
    args = (T(case["vectors"]), T(case["query"]), T(case["cs"]), T(case["sz"]), T(case["npl"]))
    with pytest.raises(AssertionError):
        IVFFlatTopkHip()(*args, 1025)
    with pytest.raises(AssertionError):
        IVFFlatTopkHip()(*args, 0)
    with pytest.raises(TorchPQAmdError):
        IVFFlatTopkHip()(torch.from_numpy(case["vectors"]), *args[1:], 5)     # a CPU tensor
    with pytest.raises(TorchPQAmdError, match="workspace"):                    # the library allocates nothing
        from torchpq_amd._lib import check, load, ptr, stream_ptr
        v, a = torch.empty(2, 5, device=DEV), torch.empty(2, 5, device=DEV, dtype=torch.long)
        check(load().tpq_ivfflat_scan_topk(ptr(args[0]), ptr(args[1]), None, ptr(args[2]), ptr(args[3]), ptr(args[4]),
                                           ptr(v), ptr(a), args[0].shape[1], 8, 2, 2, 5, 0, 4, None, 0,
                                           stream_ptr(DEV)), "tpq_ivfflat_scan_topk")


@pytest.mark.parametrize("n_split", [1, 4])
def test_scan_under_a_captured_graph(n_split):
    """replay equals eager (the process keeps its default number of hardware queues)"""
    from torchpq_amd.kernels import IVFFlatTopkHip
    case = _case(21, 64, 40, 8)
    op = IVFFlatTopkHip()
    args = (T(case["vectors"]), T(case["query"]), T(case["cs"]), T(case["sz"]), T(case["npl"]), 100)
    kw = dict(is_empty=T(case["is_empty"]), n_split=n_split)
    eager = op(*args, **kw)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        op(*args, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = op(*args, **kw)
    for _ in range(2):
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        for got, want in zip(out, eager):
            assert torch.equal(got, want)


# ---- the index -----------------------------------------------------------------------------------------
def _integer_clustered(seed, d, n, nq):
    """SIFT-like integer components 0 ... 218 around 40 centres: fp32 sums are exact (d = 32)"""
    rng = np.random.default_rng(seed)
    centers = rng.integers(30, 190, (d, 40))
    base = np.clip(centers[:, rng.integers(0, 40, n)] + rng.integers(-28, 29, (d, n)), 0, 218).astype(np.float32)
    queries = np.clip(base[:, rng.choice(n, nq, replace=False)] + rng.integers(-5, 6, (d, nq)), 0, 218)
    return base, queries.astype(np.float32)


def _build(distance="euclidean", d=32, n_cells=32, n=3000, seed=0, integer=False, nq=40):
    """train, add in three batches with explicit ids, remove some ids"""
    from torchpq_amd import util
    from torchpq_amd.index import IVFFlatIndex
    base, queries = (_integer_clustered if integer else _clustered)(seed, d, n, nq)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFFlatIndex(d, n_cells=n_cells, initial_size=16, distance=distance, device=DEV)
    idx.train(T(base))
    ids = torch.arange(n, device=DEV) * 2 + 5
    cuts = [0, n // 4, n // 2, n]
    stored = []          # what add() keeps: the batch itself, normalised as a batch for "cosine"
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = idx.add(T(base[:, lo:hi]), ids=ids[lo:hi])
        assert torch.equal(got, ids[lo:hi])
        stored.append(N(util.normalize(T(base[:, lo:hi]))) if distance == "cosine" else base[:, lo:hi])
    idx.stored_for_test = np.concatenate(stored, axis=1)
    removed = np.arange(7, n, 11)
    idx.remove(ids=ids[T(removed)])
    alive = np.ones(n, bool)
    alive[removed] = False
    return idx, base, queries, N(ids), alive


def _expected(idx, queries, k):
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    _, cells, npl = idx.probe(T(x))
    return forc.search(x, N(idx._storage), N(idx._is_empty), N(idx._cell_start), N(idx._cell_size),
                       N(idx._address2id), N(cells), N(npl), k, idx.distance)


def _check_search(idx, queries, k):
    v, i, a = idx.search(T(queries), k=k, return_address=True)
    ev, ei, ea = _expected(idx, queries, k)
    assert v.shape == (queries.shape[1], k) and v.dtype == torch.float32 and i.dtype == torch.int64
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(N(i), ei)
    v2, i2 = idx.search(T(queries), k=k)
    assert torch.equal(v2, v) and torch.equal(i2, i)
    return N(v), N(i)


@pytest.fixture(scope="module")
def built():
    return {dist: _build(dist) for dist in ("euclidean", "cosine")}


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_index_layout_and_search_against_the_oracle(built, distance):
    idx, base, queries, ids, alive = built[distance]
    assert idx._storage.shape == (32, idx.capacity, 4) and idx._storage.dtype == torch.uint8
    assert idx.code_size == 128 and idx.n_items == int(alive.sum())
    assert idx._storage.view(torch.float32).shape == (32, idx.capacity, 1)
    for n_probe, k in ((1, 1), (4, 10), (32, 100)):
        idx.n_probe = n_probe
        v, i = _check_search(idx, queries, k)
        assert not np.isin(i[i >= 0], ids[~alive]).any()          # removed ids never come back
    idx.use_smart_probing = False
    idx.n_probe = 4
    _check_search(idx, queries, 10)
    idx.use_smart_probing = True
    idx.max_query_batch = 16                                       # three batches of queries
    _check_search(idx, queries, 10)
    idx.max_query_batch = 32768
    with pytest.raises(NotImplementedError):
        idx.graphed_search(8, 10)


def test_exact_with_every_cell_probed_on_integer_data():
    """n_probe = n_cells, integer-valued data: the ids are float64 brute force over the live vectors, exactly"""
    idx, base, queries, ids, alive = _build(integer=True, seed=3)
    idx.n_probe = idx.n_cells
    idx.use_smart_probing = False
    k = 50
    v, i = _check_search(idx, queries, k)
    # float64 brute force over the live vectors; equal values are ordered by slot address, the scan's tie rule
    b64, q64 = base[:, alive].astype(np.float64), queries.astype(np.float64)
    live_ids = ids[alive]
    live_adr = N(idx.get_address_by_id(T(live_ids)))
    assert np.all(live_adr >= 0) and len(np.unique(live_adr)) == len(live_adr)
    ties = 0
    for q in range(queries.shape[1]):
        diff = q64[:, q:q + 1] - b64
        exact = -(diff * diff).sum(0)
        assert np.abs(exact).max() < 2 ** 24
        order = np.lexsort((live_adr, -exact))[:k]
        assert np.array_equal(i[q], live_ids[order])
        assert np.array_equal(v[q].astype(np.float64), exact[order])
        ties += int((exact[order][1:] == exact[order][:-1]).sum())
    print(f"{ties} ties inside the {queries.shape[1]} x {k} results")


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_expand_state_dict_and_reconstruct(built, distance):
    from torchpq_amd import util
    from torchpq_amd.index import IVFFlatIndex
    idx, base, queries, ids, alive = _build(distance, seed=1)
    idx.n_probe = 6
    before = _check_search(idx, queries, 20)
    idx.expand(torch.arange(0, idx.n_cells, 3, device=DEV))        # addresses move, results do not
    after = _check_search(idx, queries, 20)
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
    # reconstruct: the added vectors bit for bit (normalised for cosine); zero columns for removed / unknown ids
    stored = idx.stored_for_test
    ask = np.concatenate([ids, [-1, 10 ** 9]])
    rec = N(idx.reconstruct(ids=T(ask)))
    assert rec.shape == (32, len(ask)) and rec.dtype == np.float32
    assert np.array_equal(rec[:, :len(ids)][:, alive].view(np.uint32), stored[:, alive].view(np.uint32))
    assert not rec[:, :len(ids)][:, ~alive].any() and not rec[:, len(ids):].any()
    adr = idx.get_address_by_id(T(ids[alive][:50]))
    assert np.array_equal(N(idx.reconstruct(address=adr)), stored[:, alive][:, :50])
    # state_dict into a fresh index
    state = {k: v.clone() for k, v in idx.state_dict().items()}
    assert {"_storage", "_cell_start", "_cell_size", "_cell_capacity", "_is_empty", "_address2id",
            "vq_codec.kmeans.centroids"} <= set(state)
    assert all(k.startswith(("_", "vq_codec.")) for k in state)    # the container's buffers plus vq_codec.*
    fresh = IVFFlatIndex(32, n_cells=32, initial_size=16, distance=distance, device=DEV)
    fresh.load_state_dict(state)
    fresh.n_probe = 6
    # (`_max_id` is not part of the state_dict: the container recovers it as the largest stored id)
    assert fresh.capacity == idx.capacity and fresh.n_items == idx.n_items and fresh.max_id == ids[alive].max()
    again = _check_search(fresh, queries, 20)
    assert np.array_equal(again[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(again[1], after[1])
    more = fresh.add(T(base[:, :40]))                              # default ids continue after max_id
    assert int(more[0]) == ids[alive].max() + 1 and fresh.n_items == idx.n_items + 40
    _check_search(fresh, queries, 20)
