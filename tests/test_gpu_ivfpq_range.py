"""GPU: IVFPQIndex range search (tpq_ivfpq_range_count / _fill and their residual forms) against
tests/ivfpq_range_oracle.py -- lims equal, addresses equal and in the same order, values bit-equal -- on the inputs of
tests/ivfpq_range_cases.py (whose conditions tests/test_ivfpq_range_cpu.py asserts), and the index end to end."""
import numpy as np
import pytest
import torch

import ivfpq_range_cases as cases
import ivfpq_range_oracle as rorc
from oracle import c_oracle
from oracle import ivfpq_oracle as orc
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _same(got, want):
    (lims, v, a), (el, ev, ea) = got, want
    assert np.array_equal(lims, el)
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))


def _checked(case, lims, v, a):
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and a.dtype == torch.int64
    assert lims.shape == (case["cs"].shape[0] + 1,) and v.shape == a.shape == (int(lims[-1]),)
    return N(lims), N(v), N(a)


def _gpu(case):
    """the case's arrays on the GPU, uploaded once"""
    if "gpu" not in case:
        case["gpu"] = {k: T(v) for k, v in case.items() if isinstance(v, np.ndarray) and k not in ("n_cand",)}
    return case["gpu"]


def _thr(threshold):
    return T(threshold) if isinstance(threshold, np.ndarray) else threshold


def _run_plain(case, table, metric, threshold, n_split=None, op=None, with_empty=True):
    from torchpq_amd.kernels import IVFPQRangeHip
    g = _gpu(case)
    op = op or IVFPQRangeHip(m=case["storage"].shape[0] * 4)
    tables = dict(precomputed=g["lut"]) if table == "materialised" else dict(query=g["query"], codebook=g["codebook"])
    out = op(g["storage"], g["cs"], g["sz"], g["npl"], _thr(threshold), distance=metric,
             is_empty=g["is_empty"] if with_empty else None, n_split=n_split, **tables)
    return _checked(case, *out)


def _run_residual(case, tables, threshold, op=None, with_empty=True):
    from torchpq_amd.kernels import IVFPQRangeHip
    g = _gpu(case)
    op = op or IVFPQRangeHip(m=case["storage"].shape[0] * 4)
    if tables == "full":
        kw = dict(full=g["full"])
    elif tables == "part1":
        kw = dict(part1=g["part1"], part2=g["part2"], cells=g["cells"])
    else:
        kw = dict(query=g["query"], codebook=g["codebook"], part2=g["part2"], cells=g["cells"])
    out = op.residual(g["storage"], g["base_sims"], g["cs"], g["sz"], g["npl"], _thr(threshold),
                      is_empty=g["is_empty"] if with_empty else None, **kw)
    return _checked(case, *out)


@pytest.mark.parametrize("m,ds,table,nq,n_probe,metric", cases.PLAIN_CASES)
def test_plain_against_the_oracle(m, ds, table, nq, n_probe, metric):
    """Per-query thresholds from the oracle's own candidate values (three runs of the query when there is one), then
    -inf, +inf and NaN; every n_split gives the oracle's lims, addresses and value bits, hence the same as every other"""
    from torchpq_amd.kernels import IVFPQRangeHip
    case = cases.plain_case(m, ds, table, nq, n_probe, metric)
    op = IVFPQRangeHip(m=m)
    for thr, want in zip(case["runs"], case["want"]):
        for n_split in cases.SPLITS:
            got = _run_plain(case, table, metric, thr, n_split, op)
            print(f"m={m} nq={nq} n_split={op.last_n_split}: {len(got[2])} hits of {case['n_cand'].sum()} candidates")
            _same(got, want)
            if n_split is None:   # the wrapper splits a small batch over several workgroups, leaves a large one whole
                assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
            else:
                assert op.last_n_split == n_split
    for t, n_split in ((-np.inf, None), (-np.inf, 7), (np.inf, None), (np.nan, 5)):
        got = _run_plain(case, table, metric, float(t), n_split, op)
        _same(got, rorc.hits(case["cand"], t))
        assert len(got[2]) == (case["n_cand"].sum() if t == -np.inf else 0)


@pytest.mark.parametrize("m,ds,tables,nq,n_probe", cases.RESIDUAL_CASES)
def test_residual_against_the_oracle(m, ds, tables, nq, n_probe):
    case = cases.residual_case(m, ds, tables, nq, n_probe)
    for thr, want in zip(case["runs"], case["want"]):
        got = _run_residual(case, tables, thr)
        print(f"m={m} nq={nq} {tables}: {len(got[2])} hits of {case['n_cand'].sum()} candidates")
        _same(got, want)
    for t in (-np.inf, np.inf, np.nan):
        got = _run_residual(case, tables, float(t))
        _same(got, rorc.hits(case["cand"], t))
        assert len(got[2]) == (case["n_cand"].sum() if t == -np.inf else 0)


def test_without_a_tombstone_mask_and_mixed_special_thresholds():
    plain = cases.plain_case(16, 4, "fused", 6, 8, "euclidean")
    res = cases.residual_case(8, 4, "part1", 6, 8)
    cand_p = rorc.candidates(plain["storage"], plain["lut"], None, plain["cs"], plain["sz"], plain["npl"])
    cand_r = rorc.candidates_residual(res["storage"], res["part1"], res["part2"], res["cells"], res["base_sims"], None,
                                      res["cs"], res["sz"], res["npl"])
    for cand, with_mask in ((cand_p, plain["cand"]), (cand_r, res["cand"])):
        assert sum(len(s) for s, _ in cand) > sum(len(s) for s, _ in with_mask)           # the tombstones are back
        thr = cases.thresholds(cand)
        thr[2], thr[3] = np.nan, -np.inf
        want = rorc.hits(cand, thr)
        assert want[0][3] == want[0][2] and want[0][4] - want[0][3] == len(cand[3][0]) > 0
        if cand is cand_p:
            for n_split in (1, 6):
                _same(_run_plain(plain, "fused", "euclidean", thr, n_split, with_empty=False), want)
        else:
            _same(_run_residual(res, "part1", thr, with_empty=False), want)


def _check_prefix_is_topk(lims, v, a, tv, ta, k):
    sv, sa = rorc.sort_segments(lims, v, a)
    filled = ta[:, k - 1] >= 0
    assert filled.sum() >= 3                      # (-inf pads make the threshold -inf: every candidate)
    for q in range(len(ta)):
        n = lims[q + 1] - lims[q]
        real = int((ta[q] >= 0).sum())
        assert n >= real and (n >= k if filled[q] else n == real)
        assert np.array_equal(sa[lims[q]:lims[q] + real], ta[q][:real])
        assert np.array_equal(sv[lims[q]:lims[q] + real].view(np.uint32), tv[q][:real].view(np.uint32))


def test_cross_check_with_the_topk_scan():
    """threshold = the k-th value of the exact top-k scan (tpq_ivfpq_scan_topk / tpq_ivfpq_scan_topk_residual) on the
    same inputs: the range result sorted by (value descending, address ascending) starts with exactly the top-k row.
    (The top-k scan does not cut a cell that leaves the storage: these inputs keep every cell inside.)"""
    from torchpq_amd.kernels import IVFPQTopkHip
    plain = cases.plain_case(16, 4, "fused", 7, 8, "euclidean", over=False)
    res = cases.residual_case(8, 4, "part1", 7, 8, over=False)
    gp, gr = _gpu(plain), _gpu(res)
    for k in (1, 10, 100):
        tv, ta = IVFPQTopkHip(m=16).topk(gp["storage"], gp["lut"], gp["is_empty"], gp["cs"], gp["sz"], gp["npl"],
                                         n_candidates=k)
        lims, v, a = _run_plain(plain, "fused", "euclidean", N(tv[:, k - 1].contiguous()))
        _check_prefix_is_topk(lims, v, a, N(tv), N(ta), k)
        tv, ta = IVFPQTopkHip(m=8).topk_residual_precomputed(
            gr["storage"], gr["part1"], gr["part2"], gr["cells"], gr["base_sims"], gr["is_empty"], gr["cs"], gr["sz"],
            gr["npl"], n_candidates=k)
        for tables in ("part1", "built"):
            lims, v, a = _run_residual(res, tables, N(tv[:, k - 1].contiguous()))
            _check_prefix_is_topk(lims, v, a, N(tv), N(ta), k)


def test_a_nan_query_leaves_the_other_segments_alone():
    case = cases.plain_case(16, 4, "fused", 6, 8, "euclidean")
    thr = cases.thresholds(case["cand"])
    thr[2] = -np.inf
    clean = _run_plain(case, "fused", "euclidean", thr, 1)
    assert clean[0][3] > clean[0][2]
    dirty = dict(case, query=case["query"].copy())
    dirty.pop("gpu", None)
    dirty["query"][5, 2] = np.nan
    for n_split in (1, 3):
        lims, v, a = _run_plain(dirty, "fused", "euclidean", thr, n_split)
        assert lims[3] == lims[2]                                           # a NaN value is never a hit
        gone = clean[0][3] - clean[0][2]
        assert np.array_equal(np.delete(np.diff(lims), 2), np.delete(np.diff(clean[0]), 2))
        keep = np.r_[0:clean[0][2], clean[0][3]:clean[0][-1]]
        assert len(a) == len(clean[2]) - gone and np.array_equal(a, clean[2][keep])
        assert np.array_equal(v.view(np.uint32), clean[1][keep].view(np.uint32))


@pytest.mark.parametrize("form", ["plain", "residual"])
def test_fill_never_writes_beyond_a_segment_when_the_inputs_changed(form):
    """counts from a selective threshold, then a fill pass with -inf (every candidate a hit): each wave stores its
    first wave_count hits and nothing at or beyond the next segment's offset.  The outputs are as long as an unguarded
    fill would need, and hold a canary."""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    nq, n_probe, n_split = 5, 8, 3
    if form == "plain":
        case, m = cases.plain_case(16, 4, "fused", nq, n_probe, "euclidean"), 16
        g = _gpu(case)
        n_seg = lib.tpq_ivfpq_range_segments(nq, n_split)
        inputs = [ptr(g["storage"]), None, ptr(g["query"]), ptr(g["codebook"]), 4, 0, ptr(g["is_empty"]), ptr(g["cs"]),
                  ptr(g["sz"]), ptr(g["npl"])]
        shape = (case["storage"].shape[1], nq, n_probe, m, n_split, stream_ptr(DEV))
        count, fill, per_query = lib.tpq_ivfpq_range_count, lib.tpq_ivfpq_range_fill, n_split * 8
    else:
        case, m = cases.residual_case(8, 4, "part1", nq, n_probe), 8
        g = _gpu(case)
        n_seg = lib.tpq_ivfpq_range_residual_segments(nq, n_probe)
        inputs = [ptr(g["storage"]), ptr(g["part1"]), None, None, 0, ptr(g["part2"]), None, ptr(g["cells"]),
                  ptr(g["base_sims"]), ptr(g["is_empty"]), ptr(g["cs"]), ptr(g["sz"]), ptr(g["npl"])]
        shape = (case["storage"].shape[1], nq, n_probe, m, stream_ptr(DEV))
        count, fill, per_query = lib.tpq_ivfpq_range_residual_count, lib.tpq_ivfpq_range_residual_fill, n_probe * 8
    assert n_seg == nq * per_query
    cand = case["cand"]
    counts = torch.empty(n_seg, device=DEV, dtype=torch.int32)
    t_count, t_fill = T(cases.thresholds(cand, 2)), torch.full((nq,), -np.inf, device=DEV)
    check(count(*inputs, ptr(t_count), ptr(counts), *shape), "count")
    offsets = torch.zeros(n_seg + 1, device=DEV, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    total, n_all = int(offsets[-1]), sum(len(s) for s, _ in cand)
    assert 0 < total < n_all
    assert np.array_equal(N(offsets)[::per_query], rorc.hits(cand, N(t_count))[0])
    vals = torch.full((total + n_all,), 7.5, device=DEV)
    addr = torch.full((total + n_all,), -7, device=DEV, dtype=torch.int64)
    check(fill(*inputs, ptr(t_fill), ptr(offsets), ptr(vals), ptr(addr), *shape), "fill")
    torch.cuda.synchronize()
    assert torch.all(addr[total:] == -7) and torch.all(vals[total:] == 7.5)      # nothing beyond the last segment
    a, off = N(addr[:total]), N(offsets)
    assert np.all(a >= 0)                                                        # every counted place is written
    # each query's places hold candidates of THAT query, address-ascending within each wave's segment
    for q in range(nq):
        lo, hi = off[q * per_query], off[(q + 1) * per_query]
        assert np.isin(a[lo:hi], cand[q][0]).all()
    for s in range(n_seg):
        assert np.all(np.diff(a[off[s]:off[s + 1]]) != 0)


# ---- the index -----------------------------------------------------------------------------------------
def _build(distance, residual, precomputed=True, m=8, seed=0, nq=20, d=32, n_cells=32, n=3000):
    """train, add in three batches with explicit ids, remove some ids"""
    from torchpq_amd.index import IVFPQIndex
    base, queries = _clustered(seed, d, n, nq)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFPQIndex(d, n_subvectors=m, n_cells=n_cells, initial_size=16, distance=distance, device=DEV,
                     pq_use_residual=residual)
    idx.train(T(base))
    if residual and not precomputed:
        idx.use_precomputed = False
    ids = torch.arange(n, device=DEV) * 2 + 5
    cuts = [0, n // 4, n // 2, n]
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        assert torch.equal(idx.add(T(base[:, lo:hi]), ids=ids[lo:hi]), ids[lo:hi])
    removed = np.arange(7, n, 11)
    idx.remove(ids=ids[T(removed)])
    return idx, queries, N(ids), removed


def _expected(idx, queries, threshold):
    """tests/ivfpq_range_oracle.range_search on the index's own state and the cells its coarse step returns; the
    tables are the ones the index would hand its kernels, restated on the CPU where the arithmetic is pinned"""
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    sims, cells, npl = idx.probe(T(x))
    codebook = N(idx.pq_codec.codebook)
    lut = residual = None
    if not idx.pq_use_residual:
        lut = c_oracle.adc_lut(x, codebook, idx.distance)
    elif idx.use_precomputed:
        if idx._part2_by_cell is None:
            idx.precompute_part2()
        residual = dict(base_sims=N(sims), part1=orc.residual_part1(x, codebook), part2=N(idx._part2_by_cell))
    else:
        residual = dict(base_sims=N(sims), full=N(idx.precomputed_adc_residual(T(x), cells)))
    return rorc.range_search(N(idx._storage), N(idx._is_empty), N(idx._cell_start), N(idx._cell_size),
                             N(idx._address2id), N(cells), N(npl), threshold, lut=lut, residual=residual)


def _check_range_search(idx, queries, threshold):
    thr = _thr(threshold)
    lims, v, i, a = idx.range_search(T(queries), thr, return_address=True)
    el, ev, ei, ea = _expected(idx, queries, threshold)
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and i.dtype == a.dtype == torch.int64
    _same((N(lims), N(v), N(a)), (el, ev, ea))
    assert np.array_equal(N(i), ei) and np.all(ei >= 0)
    l2, v2, i2 = idx.range_search(T(queries), thr)                      # without the addresses
    assert torch.equal(l2, lims) and torch.equal(v2, v) and torch.equal(i2, i)
    ls, vs, is_, as_ = idx.range_search(T(queries), thr, return_address=True, sort=True)
    sv, sa, si = rorc.sort_segments(el, ev, ea, ei)
    _same((N(ls), N(vs), N(as_)), (el, sv, sa))
    assert np.array_equal(N(is_), si)
    return N(lims), N(v), N(i)


def _kth_values(idx, queries, k):
    """per-query thresholds: the k-th value of search -- at least k hits wherever search filled its row"""
    v = N(idx.search(T(queries), k=k)[0])[:, k - 1]
    return np.where(np.isfinite(v), v, np.float32(-1e30)).astype(np.float32)


@pytest.mark.parametrize("distance,residual,precomputed", [
    ("euclidean", False, True), ("cosine", False, True), ("euclidean", True, True), ("cosine", True, True),
    ("euclidean", True, False), ("cosine", True, False)])
def test_index_range_search_after_remove_and_expand(distance, residual, precomputed):
    idx, queries, ids, removed = _build(distance, residual, precomputed, seed=2)
    assert idx.use_precomputed == (residual and precomputed)
    for n_probe, k in ((1, 1), (32, 100)):
        idx.n_probe = n_probe
        thr = _kth_values(idx, queries, k)
        lims, v, i = _check_range_search(idx, queries, thr)
        assert np.all(np.diff(lims)[thr > -1e30] >= k) and lims[-1] > 0     # search's k-th value: search's bits
        assert not np.isin(i, ids[removed]).any()                       # removed ids never come back
    idx.n_probe = 6
    thr = _kth_values(idx, queries, 20)
    before = _check_range_search(idx, queries, thr)
    _check_range_search(idx, queries, float(np.median(thr)))             # one threshold for every query
    gone = before[2][before[0][0]:before[0][1]]                          # remove what the first query found
    idx.remove(ids=T(gone))
    after = _check_range_search(idx, queries, thr)
    assert not np.isin(after[2], gone).any() and after[0][-1] < before[0][-1]
    idx.expand(torch.arange(0, idx.n_cells, 3, device=DEV))              # addresses move, the hits do not
    moved = _check_range_search(idx, queries, thr)
    assert np.array_equal(moved[0], after[0]) and np.array_equal(moved[2], after[2])
    assert np.array_equal(moved[1].view(np.uint32), after[1].view(np.uint32))
    if not residual:
        idx.max_query_batch = 7                                          # 20 queries: batches of 7, 7 and 6
        batched = _check_range_search(idx, queries, thr)
        for got, want in zip(batched, moved):
            assert np.array_equal(got, want)
        idx.max_query_batch = 32768
    empty = idx.range_search(T(queries[:, :0]), -1.0, return_address=True)
    assert empty[0].tolist() == [0] and all(t.numel() == 0 for t in empty[1:]) and len(empty) == 4
    assert empty[1].dtype == torch.float32 and empty[2].dtype == empty[3].dtype == torch.int64


def test_long_subvectors_take_the_materialised_table():
    """d_subvector = 8 is above fused_lut_max_subvector: precompute_adc's table, or ResidualPart1Hip's part1"""
    for residual in (False, True):
        idx, queries, ids, removed = _build("euclidean", residual, m=4, seed=4)
        assert idx.d_subvector > idx.fused_lut_max_subvector
        idx.n_probe = 5
        thr = _kth_values(idx, queries, 10)
        lims, v, i = _check_range_search(idx, queries, thr)
        assert np.all(np.diff(lims)[thr > -1e30] >= 10) and lims[-1] > 0


def test_packed_layout_switch_changes_nothing_and_no_scan_layout_copy_is_built():
    idx, queries, ids, removed = _build("euclidean", False, seed=3)
    idx.n_probe = 6
    idx.use_packed_layout = False
    thr = _thr(_kth_values(idx, queries, 10))                            # (search on the reference layout)
    ref = [N(t) for t in idx.range_search(T(queries), thr, return_address=True)]
    assert ref[0][-1] > 0 and idx._packed is None
    idx.use_packed_layout = True
    got = [N(t) for t in idx.range_search(T(queries), thr, return_address=True)]
    assert idx._packed is None                                           # the range route reads _scan_codes()
    for x, y in zip(got, ref):
        assert np.array_equal(x, y)
    idx.search(T(queries), k=5)
    assert idx._packed is not None                                       # (search does build it)
