"""GPU: the IVFPQ4Index list scan (tpq_ivfpq4_scan_topk) against tests/ivfpq4_oracle.py -- values bit-equal, addresses
equal -- and the index end to end (train, add, search, remove, expand, state_dict, encode / decode)."""
import numpy as np
import pytest
import torch

import ivfpq4_cases as cases
import ivfpq4_oracle as porc
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _run(case, k, distance, n_split=None, op=None, with_empty=True):
    from torchpq_amd.kernels import IVFPQ4TopkHip
    op = op or IVFPQ4TopkHip(m=case["codebook"].shape[0])
    v, a = op(T(case["storage"]), T(case["query"]), T(case["codebook"]), T(case["cs"]), T(case["sz"]), T(case["npl"]),
              k, is_empty=T(case["is_empty"]) if with_empty else None, distance=distance, n_split=n_split)
    return N(v), N(a), op


def _check(case, k, distance, n_split=None, with_empty=True):
    v, a, op = _run(case, k, distance, n_split, with_empty=with_empty)
    ev, ea = porc.scan_topk(case["storage"], case["query"], case["codebook"],
                            case["is_empty"] if with_empty else None, case["cs"], case["sz"], case["npl"], k,
                            "euclidean" if distance == "euclidean" else "inner")
    assert v.shape == ev.shape and v.dtype == np.float32 and a.dtype == np.int64
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    return v, a, op


# (m, ds, nq, n_probe, k, distance, n_split).  m = 8: one word; 24: three words, neither a power of two nor a multiple
# of the load unroll (4 + 2 + 1 paths: 56 would take all three, 24 takes two); 64: one full unroll; 256: four, and a
# table (16 KiB) larger than the finisher's lists at k <= 64; every ds, nq, k and split of the list, both metrics;
# k = 1024 is above the live candidates
KERNEL_CASES = [
    (8, 1, 3, 1, 1, "euclidean", None),
    (8, 5, 1, 8, 1024, "inner", 5),
    (8, 2, 1000, 8, 100, "euclidean", None),
    (16, 2, 3, 8, 100, "euclidean", None),
    (16, 1, 1000, 1, 10, "inner", None),
    (16, 5, 3, 4, 1024, "euclidean", 1),
    (24, 2, 1, 4, 100, "euclidean", None),
    (24, 5, 3, 8, 300, "inner", 2),
    (24, 1, 1000, 4, 10, "euclidean", None),
    (56, 1, 3, 8, 10, "inner", None),
    (64, 2, 3, 8, 100, "euclidean", None),
    (64, 2, 1000, 4, 10, "inner", None),
    (64, 1, 3, 8, 1024, "inner", 7),
    (64, 5, 1, 8, 300, "euclidean", None),
    (256, 1, 3, 8, 10, "euclidean", None),
    (256, 2, 1, 4, 1024, "inner", 7),
    (256, 5, 3, 1, 1, "inner", 1),
    (256, 1, 1000, 8, 100, "euclidean", None),
]


@pytest.mark.parametrize("m,ds,nq,n_probe,k,distance,n_split", KERNEL_CASES)
def test_scan_against_the_oracle(m, ds, nq, n_probe, k, distance, n_split):
    case = cases.case(1000 * m + 10 * ds + nq + n_probe, m, ds, nq, n_probe)
    v, a, op = _check(case, k, distance, n_split)
    # both launches run: the wrapper splits a small batch over several workgroups and leaves a large one whole
    if n_split is None:
        assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
    else:
        assert op.last_n_split == n_split
    assert np.all(v[a < 0] == -np.inf) and np.all(v[:, 1:] <= v[:, :-1])
    if k == 1024:
        assert (a >= 0).sum(1).min() < k        # k above the number of live candidates


@pytest.mark.parametrize("n_split", [None, 1])
def test_scan_when_the_summation_order_decides(n_split):
    """The codebook is -2^20 + N(0,1), ds = 1, the query all ones, inner product: a table entry is the codebook entry,
    the m = 64 partial sums reach -2^26 (ulp 8) and the order of the additions decides which slots are the best ten.
    test_ivfpq4_cpu.test_summation_order_decides_places_in_the_offset_case checks on these very inputs that a pairwise
    fp32 sum picks another top-k set than the specification's ascending chain for at least one query (seen: it does),
    so a kernel that sums in another order fails here."""
    case, k = cases.offset_case()
    _check(case, k, "inner", n_split)


def test_split_and_unsplit_agree_and_no_tombstone_mask():
    case = cases.case(77, 24, 2, 5, 8, tomb=0)
    v1, a1, _ = _check(case, 100, "euclidean", 1, with_empty=False)
    v2, a2, _ = _check(case, 100, "euclidean", 6, with_empty=False)
    assert np.array_equal(a1, a2) and np.array_equal(v1.view(np.uint32), v2.view(np.uint32))


@pytest.mark.parametrize("n_split", [1, 4])
def test_equal_codes_are_ordered_by_address(n_split):
    """every slot holds the same code: all values tie, so the k best are the k lowest live addresses probed"""
    case = cases.case(5, 16, 2, 3, 8, tomb=40, dup=False)
    case["storage"][:] = case["storage"][:, :1]
    for k in (1, 10, 100):
        v, a, _ = _check(case, k, "euclidean", n_split)
        for q in range(3):
            slots = porc.probed_slots(case["cs"][q], case["sz"][q], case["npl"][q], case["storage"].shape[1])
            slots = np.sort(slots[case["is_empty"][slots] == 0])[:k]
            assert np.array_equal(a[q, :len(slots)], slots) and len(np.unique(v[q, :len(slots)])) <= 1


def test_a_nan_query_row_leaves_the_other_rows_alone():
    case = cases.case(9, 16, 2, 6, 8)
    clean_v, clean_a, _ = _run(case, 10, "euclidean", 1)
    for n_split in (1, 3):
        dirty = dict(case, query=case["query"].copy())
        dirty["query"][5, 2] = np.nan
        v, a, _ = _check(dirty, 10, "euclidean", n_split)
        keep = [0, 1, 3, 4, 5]
        assert np.array_equal(a[keep], clean_a[keep])
        assert np.array_equal(v[keep].view(np.uint32), clean_v[keep].view(np.uint32))
        assert np.all(a[2] == -1) and np.all(np.isneginf(v[2]))   # a NaN value never enters


def test_wrapper_and_library_decline_what_they_do_not_support():
    from torchpq_amd import _lib
    from torchpq_amd._lib import TorchPQAmdError, check, load, ptr, stream_ptr
    from torchpq_amd.index import IVFPQ4Index
    from torchpq_amd.kernels import IVFPQ4TopkHip
    case = cases.case(1, 8, 2, 2, 2)
    args = (T(case["storage"]), T(case["query"]), T(case["codebook"]), T(case["cs"]), T(case["sz"]), T(case["npl"]))
    for bad_k in (0, 1025):
        with pytest.raises(AssertionError):
            IVFPQ4TopkHip(m=8)(*args, bad_k)
    with pytest.raises(AssertionError):
        IVFPQ4TopkHip(m=12)
    with pytest.raises(AssertionError):
        IVFPQ4TopkHip(m=16)(*args, 5)                                         # another m than the codebook's
    for bad_m in (4, 12, 264):
        with pytest.raises(AssertionError):
            IVFPQ4Index(bad_m * 2, n_subvectors=bad_m, n_cells=4, device=DEV)
    with pytest.raises(AssertionError):
        IVFPQ4Index(30, n_subvectors=8, n_cells=4, device=DEV)
    with pytest.raises(TorchPQAmdError):
        IVFPQ4TopkHip(m=8)(torch.from_numpy(case["storage"]), *args[1:], 5)   # a CPU tensor
    v, a = torch.empty(2, 5, device=DEV), torch.empty(2, 5, device=DEV, dtype=torch.long)

    def scan(m, k, n_split=1, ws=None, ws_bytes=0):
        return load().tpq_ivfpq4_scan_topk(ptr(args[0]), ptr(args[1]), ptr(args[2]), None, ptr(args[3]), ptr(args[4]),
                                           ptr(args[5]), ptr(v), ptr(a), args[0].shape[1], m, 2, 2, 2, k, 0, n_split,
                                           ws, ws_bytes, stream_ptr(DEV))
    for m, k in ((12, 5), (4, 5), (264, 5), (8, 0), (8, 1025)):
        assert scan(m, k) == _lib.ERR_UNSUPPORTED, (m, k)
    with pytest.raises(TorchPQAmdError, match="workspace"):                    # the library allocates nothing
        check(scan(8, 5, n_split=4), "tpq_ivfpq4_scan_topk")
    torch.cuda.synchronize()


# ---- the index -----------------------------------------------------------------------------------------
D, M, N_CELLS, N_BASE = 32, 16, 40, 4000


def _build(distance="euclidean", seed=0, nq=40):
    """train, add in three batches with explicit ids (tiny initial cells: add forces expand), remove some ids"""
    from torchpq_amd.index import IVFPQ4Index
    base, queries = _clustered(seed, D, N_BASE, nq)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFPQ4Index(D, n_subvectors=M, n_cells=N_CELLS, initial_size=16, distance=distance, device=DEV)
    idx.train(T(base))
    ids = torch.arange(N_BASE, device=DEV) * 2 + 5
    cuts = [0, N_BASE // 4, N_BASE // 2, N_BASE]
    capacities = [idx.capacity]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        got = idx.add(T(base[:, lo:hi]), ids=ids[lo:hi])
        assert torch.equal(got, ids[lo:hi])
        capacities.append(idx.capacity)
    assert capacities[-1] > capacities[0] and capacities[-1] >= N_BASE       # add() had to expand
    removed = np.arange(7, N_BASE, 11)
    idx.remove(ids=ids[T(removed)])
    alive = np.ones(N_BASE, bool)
    alive[removed] = False
    return idx, base, queries, N(ids), alive


def _expected(idx, queries, k):
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    _, cells, npl = idx.probe(T(x))
    return porc.search(x, N(idx.pq_codec.codebook), N(idx._storage), N(idx._is_empty), N(idx._cell_start),
                       N(idx._cell_size), N(idx._address2id), N(cells), N(npl), k, idx.distance)


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
    assert idx._storage.shape == (M // 8, idx.capacity, 4) and idx._storage.dtype == torch.uint8
    assert idx.code_size == M // 2 and idx.n_items == int(alive.sum())
    assert tuple(idx.pq_codec.codebook.shape) == (M, D // M, 16)
    for n_probe, k in ((1, 1), (4, 10), (N_CELLS, 100)):
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


def test_search_cells_and_k_above_the_stored_vectors(built):
    idx, base, queries, ids, alive = built["euclidean"]
    idx.n_probe = 3
    x = T(queries)
    _, cells, npl = idx.probe(x)
    v, i, a = idx.search_cells(x, cells, n_probe_list=npl, k=20, return_address=True)
    ev, ei, ea = _expected(idx, queries, 20)
    assert np.array_equal(N(a), ea) and np.array_equal(N(i), ei)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    v2, i2 = idx.search_cells(x, cells, n_probe_list=npl, k=20)
    assert torch.equal(v2, v) and torch.equal(i2, i)
    # `_extents`: the cells' (start, size) handed in by the coarse step
    v3, i3 = idx.search_cells(x, cells, n_probe_list=npl, k=20, _extents=(idx._cell_start[cells], idx._cell_size[cells]))
    assert torch.equal(v3, v) and torch.equal(i3, i)
    # k above the number of stored vectors: a small index of its own
    from torchpq_amd.index import IVFPQ4Index
    np.random.seed(3)
    small = IVFPQ4Index(D, n_subvectors=M, n_cells=4, initial_size=16, device=DEV)
    small.train(T(base[:, :400]))
    small.add(T(base[:, :400]))
    small.n_probe = 4
    small.use_smart_probing = False
    v, i = _check_search(small, queries[:, :5], 1024)
    assert np.all((i >= 0).sum(1) == 400) and np.all(np.isneginf(v[:, 400:])) and np.all(i[:, 400:] == -1)


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_expand_state_dict_encode_and_decode(distance):
    from torchpq_amd.index import IVFPQ4Index
    idx, base, queries, ids, alive = _build(distance, seed=1)
    idx.n_probe = 6
    before = _check_search(idx, queries, 20)
    idx.expand(torch.arange(0, idx.n_cells, 3, device=DEV))        # addresses move, results do not
    after = _check_search(idx, queries, 20)
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(before[1], after[1])
    # encode / decode: the packed codes are what the container holds; decode is a gather from the codebook
    x = T(base[:, :300])
    codes = idx.encode(x)
    assert codes.shape == (M // 2, 300) and codes.dtype == torch.uint8
    adr = N(idx.get_address_by_id(T(ids[:300])))
    held = N(idx.get_data_by_address(T(adr)))
    assert np.array_equal(held[:, alive[:300]], N(codes)[:, alive[:300]])
    labels = porc.unpack(np.ascontiguousarray(N(codes).reshape(M // 8, 4, 300).transpose(0, 2, 1)))   # [M, 300]
    cb = N(idx.pq_codec.codebook)
    want = cb[np.arange(M)[:, None, None], np.arange(D // M)[None, :, None], labels[:, None, :]].reshape(D, 300)
    got = N(idx.decode(codes))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # state_dict into a fresh index
    state = {k: v.clone() for k, v in idx.state_dict().items()}
    assert {"_storage", "_cell_start", "_cell_size", "_is_empty", "_address2id", "vq_codec.kmeans.centroids",
            "pq_codec.kmeans.centroids"} <= set(state)
    fresh = IVFPQ4Index(D, n_subvectors=M, n_cells=N_CELLS, initial_size=16, distance=distance, device=DEV)
    fresh.load_state_dict(state)
    fresh.n_probe = 6
    assert fresh.capacity == idx.capacity and fresh.n_items == idx.n_items
    again = _check_search(fresh, queries, 20)
    assert np.array_equal(again[0].view(np.uint32), after[0].view(np.uint32)) and np.array_equal(again[1], after[1])
    more = fresh.add(T(base[:, :40]))                              # default ids continue after max_id
    assert int(more[0]) == ids[alive].max() + 1 and fresh.n_items == idx.n_items + 40
    _check_search(fresh, queries, 20)
    # the knobs of the codecs: settable before training only
    fresh2 = IVFPQ4Index(D, n_subvectors=M, n_cells=N_CELLS, device=DEV)
    fresh2.pq_codec_max_iter = 3
    fresh2.vq_codec_max_iter = 4
    assert fresh2.pq_codec.kmeans.max_iter == 3 and fresh2.vq_codec.kmeans.max_iter == 4
    with pytest.raises(AssertionError):
        idx.pq_codec_max_iter = 3
