"""GPU: the IVFPQ4Index list scan over residual codes (tpq_ivfpq4_scan_residual_topk) against
tests/ivfpq4_residual_oracle.py -- values bit-equal, addresses equal --, the index with pq_use_residual=True end to end
(train, add, search, remove, expand, state_dict, encode / decode), and what residual codes buy in recall."""
import numpy as np
import pytest
import torch

import ivfpq4_oracle as porc
import ivfpq4_residual_cases as cases
import ivfpq4_residual_oracle as rorc
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _run(case, k, distance, n_split=None, op=None, with_empty=True):
    from torchpq_amd.kernels import IVFPQ4ResidualTopkHip
    op = op or IVFPQ4ResidualTopkHip(m=case["codebook"].shape[0])
    v, a = op(T(case["storage"]), T(case["query"]), T(case["codebook"]), T(case["centroids"]), T(case["cells"]),
              T(case["cs"]), T(case["sz"]), T(case["npl"]), k, is_empty=T(case["is_empty"]) if with_empty else None,
              distance=distance, n_split=n_split)
    return N(v), N(a), op


def _check(case, k, distance, n_split=None, with_empty=True, expected=None):
    v, a, op = _run(case, k, distance, n_split, with_empty=with_empty)
    ev, ea = expected or cases.scan(case, k, distance, with_empty)
    assert v.shape == ev.shape and v.dtype == np.float32 and a.dtype == np.int64
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    return v, a, op


# (m, ds, nq, n_probe, k, distance, n_split).  m = 8: one word; 24: 2 + 1 tail words; 56: 4 + 2 + 1; 64: one full
# unroll; 256: four, and table buffers (two tables each at m = 256, eight at m <= 64) larger than the finisher's lists
# at k <= 512; every ds, nq, n_probe, k and split of the list, both metrics; k = 1024 is above the live candidates;
# n_split = 5 and 7 cut the 16 tiles of eight probes inside cells; n_probe = 8 at m = 256 takes four groups of tables
KERNEL_CASES = [
    (8, 1, 3, 1, 1, "euclidean", None),
    (8, 5, 1, 8, 1024, "inner", 5),
    (8, 2, 1000, 8, 100, "euclidean", None),
    (24, 2, 1, 4, 100, "euclidean", None),
    (24, 5, 3, 8, 300, "inner", 5),
    (24, 1, 1000, 4, 10, "euclidean", None),
    (56, 1, 3, 8, 10, "inner", None),
    (56, 2, 3, 4, 100, "euclidean", 7),
    (56, 5, 1, 1, 1, "inner", 1),
    (64, 2, 3, 8, 100, "euclidean", None),
    (64, 2, 1000, 4, 10, "inner", None),
    (64, 1, 3, 8, 1024, "inner", 7),
    (64, 5, 1, 8, 300, "euclidean", None),
    (64, 1, 3, 4, 10, "euclidean", 1),
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


@pytest.mark.parametrize("n_split", [1, 4, 7])
def test_every_tile_is_looked_up_in_its_own_probes_table(n_split):
    """every slot holds the same code, so a value depends on the probe's centroid alone: within a cell all values
    tie and addresses ascend, and a wave that looks a tile up in a neighbouring probe's table gives a whole tile of
    another cell's value -- which fails here and nowhere else.  The 300-slot cell spans 5 tiles, so with n_split = 7
    parts begin inside a cell."""
    case = cases.case(5, 16, 2, 3, 8, tomb=40, dup=False)
    case["storage"][:] = case["storage"][:, :1]
    cap = case["storage"].shape[1]
    for k in (1, 10, 100):
        v, a, _ = _check(case, k, "euclidean", n_split)
        for q in range(3):
            got = a[q][a[q] >= 0]
            if len(got) == 0:
                continue
            cell_of = {}
            for p, s in zip(*rorc.probe_slots(case["cs"][q], case["sz"][q], case["npl"][q], cap)):
                cell_of[int(s)] = int(case["cells"][q, p])
            by_cell = np.array([cell_of[int(s)] for s in got])
            vq = v[q][:len(got)]
            for c in np.unique(by_cell):
                assert len(np.unique(vq[by_cell == c])) == 1                     # one value per cell
                assert np.all(np.diff(got[by_cell == c]) > 0)                    # addresses ascend within it
    assert len(np.unique(v[0][a[0] >= 0])) > 1                                   # (and the cells' values differ)


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_zero_centroids_give_the_plain_scan_bit_for_bit(distance):
    from torchpq_amd.kernels import IVFPQ4TopkHip
    case = cases.case(321, 24, 2, 5, 8)
    case["centroids"][:] = 0.0
    for n_split in (1, 3):
        v, a, _ = _run(case, 100, distance, n_split)
        pv, pa = IVFPQ4TopkHip(m=24)(T(case["storage"]), T(case["query"]), T(case["codebook"]), T(case["cs"]),
                                     T(case["sz"]), T(case["npl"]), 100, is_empty=T(case["is_empty"]),
                                     distance=distance, n_split=n_split)
        assert np.array_equal(a, N(pa)) and np.array_equal(v.view(np.uint32), N(pv).view(np.uint32))
        assert (a >= 0).any()


def test_split_and_unsplit_agree_and_no_tombstone_mask():
    case = cases.case(77, 24, 2, 5, 8, tomb=0)
    expected = cases.scan(case, 100, "euclidean", with_empty=False)
    v1, a1, _ = _check(case, 100, "euclidean", 1, with_empty=False, expected=expected)
    v2, a2, _ = _check(case, 100, "euclidean", 6, with_empty=False, expected=expected)
    assert np.array_equal(a1, a2) and np.array_equal(v1.view(np.uint32), v2.view(np.uint32))


@pytest.mark.parametrize("n_split", [None, 1])
def test_scan_when_the_summation_order_decides(n_split):
    """The codebook is -2^20 + N(0,1) and every centroid component -2^20, ds = 1, the query all ones, inner product: a
    table entry is centroid + codebook exactly, the m = 64 partial sums reach -2^27 (ulp 16) and the order of the
    additions decides which slots are the best ten.  test_ivfpq4_residual_cpu.
    test_summation_order_decides_places_in_the_offset_case checks on these very inputs that a pairwise fp32 sum picks
    another top-k set than the specification's ascending chain for at least one query (seen: it does), so a kernel
    that sums in another order fails here."""
    case, k = cases.offset_case()
    _check(case, k, "inner", n_split)


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


def test_library_declines_what_it_does_not_support():
    from torchpq_amd import _lib
    from torchpq_amd._lib import TorchPQAmdError, check, load, ptr, stream_ptr
    case = cases.case(1, 8, 2, 2, 2)
    t = {key: T(val) for key, val in case.items()}
    v, a = torch.empty(2, 5, device=DEV), torch.empty(2, 5, device=DEV, dtype=torch.long)

    def scan(m=8, k=5, n_cells=len(cases.CELL_SIZES), n_split=1):
        return load().tpq_ivfpq4_scan_residual_topk(
            ptr(t["storage"]), ptr(t["query"]), ptr(t["codebook"]), ptr(t["centroids"]), ptr(t["cells"]), n_cells,
            None, ptr(t["cs"]), ptr(t["sz"]), ptr(t["npl"]), ptr(v), ptr(a), t["storage"].shape[1], m, 2, 2, 2, k, 0,
            n_split, None, 0, stream_ptr(DEV))
    for m, k in ((12, 5), (4, 5), (264, 5), (8, 0), (8, 1025)):
        assert scan(m, k) == _lib.ERR_UNSUPPORTED, (m, k)
    assert scan(n_cells=0) == -1
    with pytest.raises(TorchPQAmdError, match="workspace"):                    # the library allocates nothing
        check(scan(n_split=4), "tpq_ivfpq4_scan_residual_topk")
    assert scan() == 0
    torch.cuda.synchronize()
    ev, ea = cases.scan(case, 5, "euclidean", with_empty=False)
    assert np.array_equal(N(a), ea) and np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))


# ---- the index -----------------------------------------------------------------------------------------
D, M, N_CELLS, N_BASE = 32, 16, 40, 4000


def _build(distance="euclidean", seed=0, nq=40, pq_use_residual=True):
    """train, add in three batches with explicit ids (tiny initial cells: add forces expand), remove some ids"""
    from torchpq_amd.index import IVFPQ4Index
    base, queries = _clustered(seed, D, N_BASE, nq)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFPQ4Index(D, n_subvectors=M, n_cells=N_CELLS, initial_size=16, distance=distance, device=DEV,
                      pq_use_residual=pq_use_residual)
    train = T(base)
    kept = train.clone()
    idx.train(train)
    assert torch.equal(train, kept)                                          # the caller's tensor is left as it is
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
    state = (N(idx._storage), N(idx._is_empty), N(idx._cell_start), N(idx._cell_size), N(idx._address2id), N(cells),
             N(npl), k, idx.distance)
    if idx.pq_use_residual:
        centroids = np.ascontiguousarray(N(idx.vq_codec.codebook).T)
        return rorc.search(x, N(idx.pq_codec.codebook), centroids, *state)
    return porc.search(x, N(idx.pq_codec.codebook), *state)


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
def test_index_search_against_the_oracle(built, distance):
    idx, base, queries, ids, alive = built[distance]
    assert idx.pq_use_residual and idx._storage.shape == (M // 8, idx.capacity, 4)
    assert idx.n_items == int(alive.sum())
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
    v3, i3 = idx.search_cells(x, cells, n_probe_list=npl, k=20, _extents=(idx._cell_start[cells], idx._cell_size[cells]))
    assert torch.equal(v3, v) and torch.equal(i3, i)
    # k above the number of stored vectors: a small index of its own
    from torchpq_amd.index import IVFPQ4Index
    np.random.seed(3)
    small = IVFPQ4Index(D, n_subvectors=M, n_cells=4, initial_size=16, device=DEV, pq_use_residual=True)
    small.train(T(base[:, :400]))
    small.add(T(base[:, :400]))
    small.n_probe = 4
    small.use_smart_probing = False
    v, i = _check_search(small, queries[:, :5], 1024)
    assert np.all((i >= 0).sum(1) == 400) and np.all(np.isneginf(v[:, 400:])) and np.all(i[:, 400:] == -1)


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_state_dict_encode_decode_and_a_changed_coarse_codebook(distance):
    from torchpq_amd.index import IVFPQ4Index
    idx, base, queries, ids, alive = _build(distance, seed=1)
    idx.n_probe = 6
    before = _check_search(idx, queries, 20)
    # encode / decode: the pair (pq_code, vq_code); the packed codes are what the container holds; decode is
    # centroid + codeword, one fp32 add
    x = T(base[:, :300])
    pq_code, vq_code = idx.encode(x)
    assert pq_code.shape == (M // 2, 300) and pq_code.dtype == torch.uint8
    assert vq_code.shape == (300,) and vq_code.dtype == torch.int64
    adr = N(idx.get_address_by_id(T(ids[:300])))
    held = N(idx.get_data_by_address(T(adr)))
    assert np.array_equal(held[:, alive[:300]], N(pq_code)[:, alive[:300]])
    want = N(idx.vq_codec.decode(vq_code) + idx.pq_codec.decode(pq_code))
    got = N(idx.decode((pq_code, vq_code)))
    assert got.dtype == np.float32 and got.shape == (D, 300) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    cen = N(idx.vq_codec.codebook)[:, N(vq_code)]
    assert np.array_equal(want.view(np.uint32), (cen + N(idx.pq_codec.decode(pq_code))).view(np.uint32))
    # ... and residual codes reconstruct better than the codewords alone would
    xp = N(idx._prepare(x))
    assert np.square(got - xp).sum() < 0.5 * np.square(cen - xp).sum()
    # state_dict into a fresh index built with the same flag; the centroid copy is not part of it
    state = {k: v.clone() for k, v in idx.state_dict().items()}
    assert {"_storage", "_cell_start", "_cell_size", "_is_empty", "_address2id", "vq_codec.kmeans.centroids",
            "pq_codec.kmeans.centroids"} <= set(state)
    idx._cell_major_centroids()
    assert set(idx.state_dict()) == set(state) and sum(v.numel() for v in idx.state_dict().values()) == sum(
        v.numel() for v in state.values())
    fresh = IVFPQ4Index(D, n_subvectors=M, n_cells=N_CELLS, initial_size=16, distance=distance, device=DEV,
                        pq_use_residual=True)
    fresh.load_state_dict(state)
    fresh.n_probe = 6
    assert fresh.capacity == idx.capacity and fresh.n_items == idx.n_items
    again = _check_search(fresh, queries, 20)
    assert np.array_equal(again[0].view(np.uint32), before[0].view(np.uint32)) and np.array_equal(again[1], before[1])
    # the cached cell-major centroids follow the coarse codebook
    rows = fresh._cell_major_centroids()
    assert rows.shape == (N_CELLS, D) and fresh._cell_major_centroids() is rows
    with torch.no_grad():
        fresh.vq_codec.codebook.mul_(1.5)
    assert fresh._cell_major_centroids() is not rows
    _check_search(fresh, queries, 20)


def test_a_plain_index_still_matches_the_plain_oracle():
    idx, base, queries, ids, alive = _build("euclidean", seed=2, pq_use_residual=False)
    assert not idx.pq_use_residual
    idx.n_probe = 5
    _check_search(idx, queries, 10)
    codes = idx.encode(T(base[:, :50]))
    assert torch.is_tensor(codes) and codes.shape == (M // 2, 50)
    assert idx.decode(codes).shape == (D, 50)


def test_residual_codes_raise_recall():
    """d = 32, m = 16, 20 000 vectors around 16 centres (N(0,1) x 4, noise N(0,1)), 32 cells, n_probe 8, 200 queries =
    stored vectors + 0.3 N(0,1), recall@10 against FlatIndex.search: the residual index and a plain one share the coarse
    codebook.  A NumPy stand-in (plain k-means) gave 0.63 against 0.21; the margin of 0.1 leaves four fifths of that gap
    for the difference between the two k-means."""
    from torchpq_amd.index import FlatIndex, IVFPQ4Index
    base, queries = _clustered(11, 32, 20000, 200, n_centers=16, spread=4.0)
    xb, xq = T(base), T(queries)
    np.random.seed(11)
    torch.manual_seed(11)
    kw = dict(n_subvectors=16, n_cells=32, initial_size=1024, device=DEV)
    plain = IVFPQ4Index(32, **kw)
    resid = IVFPQ4Index(32, pq_use_residual=True, **kw)
    plain.train(xb)
    resid.vq_codec.load_state_dict(plain.vq_codec.state_dict())
    resid.pq_codec.train(resid._residual(xb, resid.vq_codec.encode(xb)))
    assert torch.equal(resid.vq_codec.codebook, plain.vq_codec.codebook)
    flat = FlatIndex(32, initial_size=20000, device=DEV)
    for idx in (plain, resid, flat):
        idx.add(xb)
    _, truth = flat.search(xq, k=10)
    recall = {}
    for name, idx in (("plain", plain), ("residual", resid)):
        idx.n_probe = 8
        idx.use_smart_probing = False
        _, ids = idx.search(xq, k=10)
        recall[name] = float(np.mean([len(set(a) & set(b)) / 10.0 for a, b in zip(N(ids).tolist(), N(truth).tolist())]))
    print(f"recall@10: residual {recall['residual']:.3f}, plain {recall['plain']:.3f}")
    assert recall["residual"] >= recall["plain"] + 0.1, recall
