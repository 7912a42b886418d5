"""GPU: the re-rank kernel (tpq_ivfpqr_rerank) and IVFPQRIndex where the first tests (test_gpu_ivfpqr.py) do not
reach -- sub-vectors that cross the kernel's 16-dimension slices, workgroup boundaries, non-finite values, every
first-stage route at large k, stale packed copies, arenas, tombstones, the small ends.  Same standard: values
bit-equal to tests/ivfpqr_oracle.py, addresses and ids equal."""
import io

import numpy as np
import pytest
import torch

import ivfpqr_oracle as rorc
from tests_support import DEV, N, T, _case, _check_search, _clustered, _expected_search, _run_and_compare

pytestmark = pytest.mark.gpu

MODES = [(True, "euclidean"), (True, "cosine"), (False, "euclidean"), (False, "cosine")]

# ---- A. the kernel -------------------------------------------------------------------------------------
# (m, m_r, d): (ds, ds_r) = (32, 32), (120, 240), (50, 25) with d % 16 = 8, (30, 10), (2, 32), (32, 2), and
# (1, 1) at util.max_subvectors().  ORACLE_SHAPES of test_ivfpqr_cpu.py ties the oracle to float64 at each.
SLICE_SHAPES = [(4, 4, 128), (8, 4, 960), (4, 8, 200), (4, 12, 120), (64, 4, 128), (4, 64, 128), (152, 152, 152)]
SLICE_K1_K = [(7, 3), (200, 100), (1024, 512)]


def _scale_of(d):
    return 0.25 if d >= 960 else None   # keeps |value| of the long vectors near that of the short ones


def test_the_largest_shape_is_the_subvector_limit():
    from torchpq_amd import util
    assert util.max_subvectors() == SLICE_SHAPES[-1][0]


@pytest.mark.parametrize("use_residual,distance", MODES)
@pytest.mark.parametrize("m,m_r,d", SLICE_SHAPES)
def test_rerank_kernel_subvectors_across_slices(m, m_r, d, use_residual, distance):
    for k1, k in SLICE_K1_K:
        for nq in (1, 3, 200):
            cap = max(1500, k1 + 100)
            case = _case(1000 * k1 + nq + m + d, m, m_r, d, cap, nq, k1, distance, scale=_scale_of(d))
            v, a, _ = _run_and_compare(*case, k, use_residual, distance, m)
            assert np.isfinite(v[a >= 0]).all()


def _queries_per_group(k1):
    return min(64, max(1, 1024 // k1))   # csrc/rerank.hip queries_per_group


@pytest.mark.parametrize("k1", [15, 17, 33, 341, 513, 1000])
def test_rerank_kernel_workgroup_boundaries(k1):
    """a full last workgroup (nq == group), a partial one (2 * group + 1 queries), k = 1 and k = k1"""
    m, m_r, d = 16, 32, 64
    group = _queries_per_group(k1)
    assert group == {15: 64, 17: 60, 33: 31, 341: 3, 513: 1, 1000: 1}[k1]
    for use_residual, distance in MODES:
        for nq in (group, 2 * group + 1):
            case = _case(77 * k1 + nq, m, m_r, d, 2000, nq, k1, distance)
            for k in (1, k1):
                _run_and_compare(*case, k, use_residual, distance, m)


def _assert_real_minus_inf_before_padding(vals, adr, ids, k):
    """the structure the -inf cases are built for; returns how many real candidates carry -inf"""
    n_real_inf, rows_with_both = 0, 0
    for q in range(vals.shape[0]):
        real = adr[q] >= 0
        n_real = int(real.sum())
        assert real[:n_real].all() and not real[n_real:].any()          # padding comes last
        assert np.all(np.isneginf(vals[q, n_real:])) and np.all(ids[q, n_real:] == -1)
        assert np.all(ids[q, :n_real] >= 0)
        inf_real = np.isneginf(vals[q]) & real
        pos = np.nonzero(inf_real)[0]
        if pos.size:
            assert pos[-1] == n_real - 1 and pos.size == pos[-1] - pos[0] + 1   # one run, just before the padding
            assert np.all(np.diff(adr[q, pos]) > 0)                             # by address among themselves
            assert not np.isnan(vals[q]).any()
            n_real_inf += pos.size
            rows_with_both += int(n_real < k)
    return n_real_inf, rows_with_both


def _minus_inf_case(use_residual, distance, how):
    """k1 = 64 candidates, k = 48.  `how` = "codes": three code values of re-rank sub-quantizer 0 decode to entries so
    large that the value overflows, and every row's candidates at positions 2, 5, 8, ... 29 carry one of them;
    "query" (euclidean): columns 2 and 5 of the query are 1e20, every square overflows.  Rows 0, 2 and 5 keep 20, 30
    and 40 real candidates: fewer than k, so real -inf candidates stand next to padding."""
    m, m_r, d, cap, nq, k1 = 8, 8, 32, 1500, 8, 64
    storage, cb, cb_r, query, cand, a2i = _case(31, m, m_r, d, cap, nq, k1, distance)
    cand = np.argsort(np.random.default_rng(32).random((nq, cap)), axis=1)[:, :k1].astype(np.int64)
    hot = np.array([3, 77, 200])
    if how == "codes":
        if distance == "euclidean":
            cb_r[0][:, hot] = 1e30           # (q - r)^2 and |c|^2 overflow
        else:
            cb_r[0][:, hot] = -3e38          # q * r overflows downwards for q = 2
            query[:d // m_r] = 2.0
        col = storage[m // 4, :, 0]          # (a view) code of re-rank sub-quantizer 0, per slot
        col[np.isin(col, hot)] = 9           # no slot carries one of them by chance ...
        for q in range(nq):                  # ... the chosen candidates do
            for j, c in enumerate(range(2, 30, 3)):
                col[cand[q, c]] = hot[j % 3]
    else:
        assert distance == "euclidean"
        query[:, [2, 5]] = 1e20
    for q, n_real in ((0, 20), (2, 30), (5, 40)):
        cand[q, n_real:] = -1
    cand[7, ::2] = -1                        # holes anywhere in the row
    return storage, cb, cb_r, query, cand, a2i, m


@pytest.mark.parametrize("use_residual,distance,how", [(r, dist, "codes") for r, dist in MODES]
                         + [(True, "euclidean", "query"), (False, "euclidean", "query")])
def test_rerank_kernel_minus_inf_is_a_value(use_residual, distance, how):
    """a real candidate whose value is -inf is a candidate: it carries its address and id, ranks by address among
    its like, and stands ahead of the (-inf, -1, -1) padding"""
    k = 48
    storage, cb, cb_r, query, cand, a2i, m = _minus_inf_case(use_residual, distance, how)
    with np.errstate(all="ignore"):
        ev, ea, ei = rorc.rerank(storage, cb, cb_r, query, cand, k, use_residual, distance, a2i)
    # the input has the structure (checked on the oracle, so it cannot silently degrade) ...
    n_real_inf, rows_with_both = _assert_real_minus_inf_before_padding(ev, ea, ei, k)
    assert n_real_inf >= 20 and rows_with_both >= 2, (n_real_inf, rows_with_both)
    # ... and the kernel gives it back
    with np.errstate(all="ignore"):
        v, a, i = _run_and_compare(storage, cb, cb_r, query, cand, a2i, k, use_residual, distance, m)
    assert _assert_real_minus_inf_before_padding(v, a, i, k) == (n_real_inf, rows_with_both)
    real_inf = np.isneginf(v) & (a >= 0)
    assert np.array_equal(i[real_inf], a2i[a[real_inf]])


@pytest.mark.parametrize("use_residual,distance", MODES)
@pytest.mark.parametrize("m,m_r,d", [(8, 8, 32), (4, 4, 128)])
def test_rerank_kernel_nan_and_inf_queries_stay_in_their_rows(m, m_r, d, use_residual, distance):
    """the list scan's contract (test_gpu_round3.py): the call returns, a finite query's row is what it is without
    the poison, a poisoned row holds -1 or its own candidates, none more often than the input row does.  k1 = 16: a
    workgroup holds 64 queries, poisoned and finite ones side by side; 130 queries leave the last one partial."""
    from torchpq_amd.kernels import IVFPQRerankHip
    nq, k1, k, cap = 130, 16, 8, 1500
    storage, cb, cb_r, query, cand, a2i = _case(41 + d, m, m_r, d, cap, nq, k1, distance)
    poisoned = [1, 3, 4, 6, 7, 69, 128]
    full = np.argsort(np.random.default_rng(42).random((nq, cap)), axis=1)[:, :k1].astype(np.int64)
    cand[poisoned[1:]] = full[poisoned[1:]]   # row 1 has no candidate (_case); the others have theirs, ...
    cand[7, ::3] = -1                         # ... one with holes, ...
    cand[69, 3] = cand[69, 2]                 # ... one that names a slot twice
    bad = query.copy()
    bad[0, 1] = np.nan
    bad[:, 3] = np.nan
    bad[5, 4] = np.inf
    bad[2, 6] = -np.inf
    bad[:, 7] = 3.0e38                        # finite, but every square overflows
    bad[d - 1, 69] = np.nan                   # second workgroup, last dimension
    bad[17, 128] = np.inf                     # the partial last workgroup (second slice)
    args = (T(storage), m, T(cb) if use_residual else None, T(cb_r))
    kw = dict(use_residual=use_residual, distance=distance, address2id=T(a2i))
    clean = [N(t) for t in IVFPQRerankHip()(*args, T(query), T(cand), k, **kw)]
    got = IVFPQRerankHip()(*args, T(bad), T(cand), k, **kw)
    torch.cuda.synchronize()
    v, a, i = (N(t) for t in got)
    good = np.setdiff1d(np.arange(nq), poisoned)
    assert np.array_equal(v[good].view(np.uint32), clean[0][good].view(np.uint32))
    assert np.array_equal(a[good], clean[1][good]) and np.array_equal(i[good], clean[2][good])
    n_real = 0
    for q in poisoned:
        real = cand[q][cand[q] >= 0]
        n_real += real.size
        out = a[q][a[q] >= 0]
        assert np.all(a[q] >= -1) and np.isin(out, real).all(), q
        for adr, count in zip(*np.unique(out, return_counts=True)):
            assert count <= int((real == adr).sum()), (q, adr)
        assert np.array_equal(i[q], np.where(a[q] >= 0, a2i[np.maximum(a[q], 0)], -1))
    assert n_real >= 5 * k1                   # the poisoned rows do have candidates


def test_rerank_entry_point_edges():
    from torchpq_amd import _lib
    from torchpq_amd.kernels import IVFPQRerankHip
    m, m_r, d, cap, nq, k1, k = 8, 8, 16, 300, 5, 12, 6
    storage, cb, cb_r, query, cand, a2i = _case(51, m, m_r, d, cap, nq, k1, "euclidean")
    op = IVFPQRerankHip()
    # no queries: [0, k] tensors, nothing launched
    out = op(T(storage), m, T(cb), T(cb_r), T(query[:, :0]), T(cand[:0]), k, address2id=T(a2i))
    torch.cuda.synchronize()
    assert [tuple(t.shape) for t in out] == [(0, k)] * 3
    assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.int64]
    assert len(op(T(storage), m, T(cb), T(cb_r), T(query[:, :0]), T(cand[:0]), k)) == 2
    # without address2id: the first two of the three
    three = op(T(storage), m, T(cb), T(cb_r), T(query), T(cand), k, address2id=T(a2i))
    two = op(T(storage), m, T(cb), T(cb_r), T(query), T(cand), k)
    assert len(two) == 2 and torch.equal(two[0].view(torch.int32), three[0].view(torch.int32))
    assert torch.equal(two[1], three[1])
    # not use_residual needs no first-stage codebook
    for distance in ("euclidean", "cosine"):
        v, a = op(T(storage), m, None, T(cb_r), T(query), T(cand), k, use_residual=False, distance=distance)
        ev, ea, _ = rorc.rerank(storage, None, cb_r, query, cand, k, False, distance)
        assert np.array_equal(N(a), ea) and np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    # k1 = 1025: refused by the wrapper and by the library, nothing launched
    wide = np.tile(np.arange(205, dtype=np.int64), (nq, 5))
    assert wide.shape == (nq, 1025)
    with pytest.raises(AssertionError):
        op(T(storage), m, T(cb), T(cb_r), T(query), T(wide), k)
    t = [T(x) for x in (storage, cb, cb_r, query, wide)]
    v = torch.full((nq, k), 7.0, device=DEV)
    a = torch.full((nq, k), 7, device=DEV, dtype=torch.int64)
    rc = _lib.load().tpq_ivfpqr_rerank(_lib.ptr(t[0]), cap, m, m_r, _lib.ptr(t[1]), _lib.ptr(t[2]), _lib.ptr(t[3]), d,
                                       nq, _lib.ptr(t[4]), 1025, k, 1, _lib.METRIC_NEG_SQ_L2, None, _lib.ptr(v),
                                       _lib.ptr(a), None, _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    assert rc == _lib.ERR_UNSUPPORTED and "k1=1025" in _lib.last_error()
    assert torch.all(v == 7.0) and torch.all(a == 7)


# ---- B. the index --------------------------------------------------------------------------------------
N_BASE, N_QUERY = 24000, 40
_INDEXES = {}


def _index(d, m, m_r, n_cells=64, n=N_BASE, distance="euclidean", use_residual=True):
    """a trained index with `n` clustered vectors under non-contiguous ids, built once per module and shape; tests
    that change its contents take a copy (`_copy_of`)"""
    from torchpq_amd.index import IVFPQRIndex
    key = (d, m, m_r, n_cells, n, distance, use_residual)
    if key not in _INDEXES:
        base, queries = _clustered(100 + d + m, d, n, N_QUERY)
        np.random.seed(d + m)
        torch.manual_seed(d + m)
        idx = IVFPQRIndex(d, n_subvectors=m, n_subvectors_rerank=m_r, n_cells=n_cells, use_residual=use_residual,
                          initial_size=64, distance=distance, device=DEV)
        idx.set_vq_codec_max_iter(8)
        idx.set_pq_codec_max_iter(6)
        idx.set_pq_rerank_codec_max_iter(6)
        idx.train(T(base))
        ids = torch.from_numpy(np.random.default_rng(d).permutation(n) * 7 + 3).to(DEV)
        idx.add(T(base[:, :n // 2]), ids=ids[:n // 2])
        idx.add(T(base[:, n // 2:]), ids=ids[n // 2:])
        _INDEXES[key] = (idx, base, queries, ids)
    idx, base, queries, ids = _INDEXES[key]
    idx.use_packed_layout, idx.use_fused_lut, idx.use_smart_probing = True, True, True
    idx.n_probe, idx.rerank_factor, idx.max_query_batch = 8, 2, 32768
    return idx, base, queries, ids


def _copy_of(idx, **kw):
    from torchpq_amd.index import IVFPQRIndex
    fresh = IVFPQRIndex(idx.d_vector, n_subvectors=idx.n_subvectors, n_subvectors_rerank=idx.n_subvectors_rerank,
                        n_cells=idx.n_cells, use_residual=idx.use_residual, distance=idx.distance, device=DEV, **kw)
    # (load_state_dict registers the tensors it is given: clones, or the copy would write into `idx`)
    fresh.load_state_dict({k: v.clone() for k, v in idx.state_dict().items()})
    fresh.n_probe = idx.n_probe
    return fresh


def _route(idx):
    return idx._ivfpq_topk._scan.last_route()


# k1 = 1, 200 (<= 248), 400 (the pools, <= 504), 750 (<= 1016), 1024
K_FACTOR = [(1, 1), (10, 20), (100, 4), (250, 3), (256, 4)]
INDEX_SHAPES = [(128, 64, 64), (128, 16, 32), (64, 32, 16), (96, 24, 8), (128, 4, 4)]


@pytest.mark.parametrize("d,m,m_r", INDEX_SHAPES)
def test_index_shapes_layouts_and_first_stage_routes(d, m, m_r):
    idx, base, queries, ids = _index(d, m, m_r)
    assert idx.n_items == N_BASE
    routes = set()
    for packed in (True, False):
        for fused in (True, False):
            for smart in (True, False):
                idx.use_packed_layout, idx.use_fused_lut, idx.use_smart_probing = packed, fused, smart
                for k, factor in K_FACTOR:
                    idx.rerank_factor = factor
                    _check_search(idx, queries, k)
                    routes.add(_route(idx))
    print(f"d={d} m={m} m_r={m_r}: first-stage routes {sorted(routes)}")
    assert "reference_layout" in routes and len(routes) >= 2


def test_index_with_a_code_length_outside_the_packed_list():
    from torchpq_amd.kernels import PACKED_M
    d, m, m_r = 72, 36, 12
    assert m not in PACKED_M
    idx, base, queries, ids = _index(d, m, m_r, n=8000)
    for packed in (True, False):
        for fused in (True, False):
            idx.use_packed_layout, idx.use_fused_lut = packed, fused
            for k, factor in K_FACTOR:
                idx.rerank_factor = factor
                _check_search(idx, queries, k)
            assert _route(idx) == "reference_layout"


@pytest.mark.parametrize("d,m,m_r", [(128, 64, 64), (64, 32, 16)])
def test_index_large_batch(d, m, m_r):
    """1 100 queries (one batch of the large-batch route and a bit) equal the same index searched 256 at a time, row
    for row, and 64 rows spread over the batch (the last one among them) equal the oracle"""
    idx, base, queries, ids = _index(d, m, m_r)
    rng = np.random.default_rng(9)
    nq = 1100
    x = (np.tile(queries, (1, nq // N_QUERY + 1))[:, :nq] + 0.2 * rng.standard_normal((d, nq))).astype(np.float32)
    rows = np.unique(np.concatenate([np.linspace(0, nq - 1, 64).astype(np.int64), [255, 256, 1023, 1024, 1025]]))
    assert rows.size >= 64 and rows[-1] == nq - 1
    routes = set()
    for k, factor in ((50, 4), (100, 4), (250, 4)):          # k1 = 200, 400 (<= 504) and 1000 (> 504)
        idx.rerank_factor = factor
        for packed, fused in ((True, True), (True, False), (False, True)):
            idx.use_packed_layout, idx.use_fused_lut = packed, fused
            idx.max_query_batch = 32768
            v, i, a = idx.search(T(x), k=k, return_address=True)
            routes.add(_route(idx))
            assert v.shape == (nq, k) and (_route(idx) == "reference_layout") == (not packed)
            idx.max_query_batch = 256
            v2, i2, a2 = idx.search(T(x), k=k, return_address=True)
            assert torch.equal(v.view(torch.int32), v2.view(torch.int32)) and torch.equal(i, i2)
            assert torch.equal(a, a2)
            idx.max_query_batch = 32768
            ev, ei, ea = _expected_search(idx, x, k, rows=rows)
            assert np.array_equal(N(a)[rows], ea)
            assert np.array_equal(N(v)[rows].view(np.uint32), ev.view(np.uint32))
            assert np.array_equal(N(i)[rows], ei)
    print(f"m={m}: first-stage routes of the 1 100-query calls {sorted(routes)}")
    assert any(r.startswith("dump") for r in routes) and "pools" in routes   # the large-batch route did run


def _packed_is_current(idx):
    from torchpq_amd.kernels import PackCodesHip
    assert torch.equal(idx.packed_storage(), PackCodesHip()(idx._scan_codes()))


def test_packed_copy_goes_stale_on_every_write():
    """packed search -> add (no remove before it) -> packed search; the same through set_data_by_address and
    through an add that grows the container"""
    src, base, queries, ids = _index(64, 32, 16)
    idx = _copy_of(src)
    idx.use_packed_layout = True
    rng = np.random.default_rng(3)
    new = (base[:, :300] + 0.5 * rng.standard_normal((64, 300))).astype(np.float32)
    probes = np.concatenate([new[:, :20], queries[:, :20]], axis=1)

    def check(expect_ids):
        for k in (10, 100):
            _, i = _check_search(idx, probes, k)
            assert _route(idx) != "reference_layout"
        assert np.isin(i[:20, :20], expect_ids).any(axis=1).sum() >= 15   # the new vectors are found
        _packed_is_current(idx)

    _check_search(idx, probes, 10)
    assert idx._packed_valid
    # add into free slots: same capacity, the same packed tensor would be scattered into
    capacity = idx.capacity
    free = N(idx._cell_capacity - idx._cell_size)
    cells = N(idx.vq_codec.encode(T(new[:, :40])))
    assert np.all(np.bincount(cells, minlength=idx.n_cells) <= free)
    new_ids = torch.arange(40, device=DEV) + 10 ** 7
    idx.add(T(new[:, :40]), ids=new_ids)
    assert idx.capacity == capacity
    check(N(new_ids))
    # set_data_by_address directly: the codes of the first 20 new slots replaced by those of other vectors
    assert idx._packed_valid
    adr = idx.get_address_by_id(new_ids[:20])
    idx.set_data_by_address(idx.encode(T(new[:, 100:120])), adr)
    for k in (10, 100):
        _check_search(idx, np.concatenate([new[:, 100:120], queries[:, :20]], axis=1), k)
    _packed_is_current(idx)
    idx.set_data_by_address(idx.encode(T(new[:, :20])), adr)
    check(N(new_ids))
    # an add that forces growth
    many = (base[:, :12000] + 0.5 * rng.standard_normal((64, 12000))).astype(np.float32)
    many_ids = torch.arange(12000, device=DEV) + 2 * 10 ** 7
    idx.add(T(many), ids=many_ids)
    assert idx.capacity > capacity and idx.n_items == N_BASE + 40 + 12000
    probes = np.concatenate([many[:, :20], queries[:, :20]], axis=1)
    check(N(many_ids))


def test_growth_through_the_arenas():
    from torchpq_amd.index import IVFPQRIndex
    d, m, m_r = 64, 32, 16
    src, base, queries, ids = _index(d, m, m_r)
    idx = IVFPQRIndex(d, n_subvectors=m, n_subvectors_rerank=m_r, n_cells=src.n_cells, initial_size=16, device=DEV)
    for name in ("vq_codec", "pq_codec", "pq_rerank_codec"):
        getattr(idx, name).load_state_dict({k: v.clone() for k, v in getattr(src, name).state_dict().items()})
    idx.arena_min_bytes = 1                  # every growth takes the arena path
    idx.n_probe = 8
    for lo, hi in ((0, 3000), (3000, 9000), (9000, 20000)):
        idx.add(T(base[:, lo:hi]), ids=ids[lo:hi])
        assert idx._arena and idx._storage.untyped_storage().nbytes() > idx._storage.numel()
        assert tuple(idx._storage.shape) == ((m + m_r) // 4, idx.capacity, 4)
        for packed in (True, False):
            idx.use_packed_layout = packed
            for k, factor in ((10, 2), (100, 4), (256, 4)):
                idx.rerank_factor = factor
                _check_search(idx, queries, k)
    idx.rerank_factor = 2
    assert torch.equal(idx.get_data_by_address(idx.get_address_by_id(ids[:20000])), idx.encode(T(base[:, :20000])))
    buf = io.BytesIO()
    torch.save(idx.state_dict(), buf)
    buf.seek(0)
    sd = torch.load(buf, map_location="cpu")
    cap = idx.capacity
    assert tuple(sd["_storage"].shape) == ((m + m_r) // 4, cap, 4) and tuple(sd["_address2id"].shape) == (cap,)
    for name in ("_storage", "_address2id", "_is_empty"):
        assert sd[name].untyped_storage().nbytes() == sd[name].numel() * sd[name].element_size(), name
    fresh = IVFPQRIndex(d, n_subvectors=m, n_subvectors_rerank=m_r, n_cells=src.n_cells, device=DEV)
    fresh.load_state_dict(sd)
    fresh.n_probe = 8
    want = _check_search(idx, queries, 10)
    got = _check_search(fresh, queries, 10)
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)) and np.array_equal(got[1], want[1])


@pytest.mark.parametrize("d,m,m_r", [(64, 32, 16), (128, 4, 4)])
def test_tombstones_inside_cells(d, m, m_r):
    """a foreign state_dict with a tenth of the occupied slots marked empty, not compacted: the scan is handed
    `is_empty`, and the re-rank never sees a dead slot"""
    src, base, queries, ids = _index(d, m, m_r)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    rng = np.random.default_rng(13)
    occupied = np.nonzero(N(sd["_is_empty"]) == 0)[0]
    dead = np.sort(rng.choice(occupied, occupied.size // 10, replace=False))
    sd["_is_empty"][torch.from_numpy(dead).to(sd["_is_empty"].device)] = 1
    sd["_address2id"][torch.from_numpy(dead).to(sd["_address2id"].device)] = -1
    idx = _copy_of(src)
    idx.load_state_dict(sd)
    assert idx._has_holes and idx.n_probe == 8
    for packed in (True, False):
        for fused in (True, False):
            idx.use_packed_layout, idx.use_fused_lut = packed, fused
            for k, factor in ((10, 2), (100, 4), (256, 4)):
                idx.rerank_factor = factor
                v, i, a = idx.search(T(queries), k=k, return_address=True)
                assert not np.isin(N(a), dead).any()
                assert np.all((N(a) >= 0) == (N(i) >= 0))
                _check_search(idx, queries, k)
    # remove (compacts the cells) and add on top of it
    idx.use_packed_layout, idx.use_fused_lut, idx.rerank_factor = True, True, 2
    _, i = _check_search(idx, queries, 10)
    gone = torch.from_numpy(np.unique(i[:, :3][i[:, :3] >= 0])).to(DEV)
    idx.remove(ids=gone)
    assert not idx._has_holes and idx.n_items == N_BASE - dead.size - gone.numel()
    for packed in (True, False):
        idx.use_packed_layout = packed
        _, i = _check_search(idx, queries, 10)
        assert not np.isin(i, N(gone)).any()
    idx.add(T(base[:, :500]), ids=torch.arange(500, device=DEV) + 10 ** 7)
    for packed in (True, False):
        idx.use_packed_layout = packed
        for k, factor in ((10, 2), (256, 4)):
            idx.rerank_factor = factor
            _check_search(idx, queries, k)


def test_index_small_ends():
    d, m, m_r = 64, 32, 16
    src, base, queries, ids = _index(d, m, m_r)
    # no queries, one query, every cell probed -- on each layout and LUT path
    for packed in (True, False):
        for fused in (True, False):
            src.use_packed_layout, src.use_fused_lut, src.n_probe = packed, fused, 8
            for return_address in (False, True):
                out = src.search(T(queries[:, :0]), k=5, return_address=return_address)
                assert [tuple(t.shape) for t in out] == [(0, 5)] * (3 if return_address else 2)
                assert [t.dtype for t in out] == [torch.float32, torch.int64, torch.int64][:len(out)]
            _check_search(src, queries[:, :1], 10)
            src.n_probe = src.n_cells
            src.use_smart_probing = False
            _check_search(src, queries[:, :8], 100)
            src.use_smart_probing = True
    # fewer vectors than k, and k1 beyond what is stored: real hits, then (-inf, -1)
    few = _copy_of(src)
    few.empty()
    few.add(T(base[:, :30]), ids=ids[:30])
    few.n_probe, few.use_smart_probing = few.n_cells, False
    for packed in (True, False):
        few.use_packed_layout = packed
        for k, factor in ((50, 1), (50, 4), (4, 256)):
            few.rerank_factor = factor
            v, i = _check_search(few, queries[:, :6], k)
            n_hits = min(k, 30)
            assert np.all(i[:, :n_hits] >= 0) and np.all(np.isfinite(v[:, :n_hits]))
            assert np.all(i[:, n_hits:] == -1) and np.all(np.isneginf(v[:, n_hits:]))
            assert np.isin(i[:, :n_hits], N(ids[:30])).all()
