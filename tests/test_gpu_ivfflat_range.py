"""GPU: IVFFlatIndex range search (tpq_ivfflat_range_count / tpq_ivfflat_range_fill) against
tests/ivfflat_range_oracle.py -- lims equal, addresses equal and in the same order, values bit-equal -- and the index
end to end (range_search after remove and expand, batches, sort, cosine, brute force)."""
import numpy as np
import pytest
import torch

import ivfflat_oracle as forc
import ivfflat_range_oracle as rorc
from test_gpu_ivfflat import _build, _case
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu

SPLITS = (None, 1, 5, 7)


def _metric(distance):
    return "euclidean" if distance == "euclidean" else "inner"


def _range_case(seed, d, nq, n_probe, **kw):
    """the layout of the top-k scan's tests (cells of 0, 1, 63, 64, 65, 300, 17 and 128 slots with spare capacity
    behind each, tombstones inside the cells, one cell listed twice in a row, n_probe_list below, at and beyond
    max_nprobe) with, from three queries on, a last query that probes nothing"""
    case = _case(seed, d, nq, n_probe, scale=0.25 if d >= 960 else 1.0, **kw)
    if nq >= 3:
        case["npl"][-1] = 0
    return case


def _thresholds(cand, rotate=0):
    """per-query thresholds taken from the query's own candidate values, so most sit exactly ON a value: by turns the
    smallest value (every candidate is a hit), one ulp above the largest (no hit), the median, the upper decile"""
    thr = np.zeros(len(cand), np.float32)
    for q, (_, v) in enumerate(cand):
        v = np.sort(v[~np.isnan(v)])
        if len(v) == 0:
            continue
        kind = (q + rotate) % 4
        thr[q] = (v[0], np.nextafter(v[-1], np.float32(np.inf)), v[len(v) // 2], v[(9 * len(v)) // 10])[kind]
    return thr


def _run(case, threshold, distance, n_split=None, op=None, with_empty=True):
    from torchpq_amd.kernels import IVFFlatRangeHip
    op = op or IVFFlatRangeHip()
    thr = T(threshold) if isinstance(threshold, np.ndarray) else threshold
    lims, v, a = op(T(case["vectors"]), T(case["query"]), T(case["cs"]), T(case["sz"]), T(case["npl"]), thr,
                    is_empty=T(case["is_empty"]) if with_empty else None, distance=distance, n_split=n_split)
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and a.dtype == torch.int64
    assert lims.shape == (case["query"].shape[1] + 1,) and v.shape == a.shape == (int(lims[-1]),)
    return N(lims), N(v), N(a), op


def _same(got, want):
    (lims, v, a), (el, ev, ea) = got, want
    assert np.array_equal(lims, el)
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))


def _assert_not_vacuous(hits, n_cand):
    """the condition on a case's inputs, asserted on the oracle before the kernel runs: a query with zero hits, a query
    whose every live candidate is a hit (and that has candidates), hits at all"""
    assert (hits == 0).any() and ((hits == n_cand) & (n_cand > 0)).any() and hits.sum() > 0, (hits, n_cand)


# (d, nq, n_probe, distance): every d (the unroll tail, 3 and 1; multiples of the unroll), both metrics per d, every nq
RANGE_CASES = [
    (1, 3, 4, "euclidean"),
    (1, 1000, 8, "inner"),
    (3, 1, 8, "inner"),
    (3, 1000, 8, "euclidean"),
    (24, 3, 8, "euclidean"),
    (24, 1000, 1, "inner"),
    (128, 1, 8, "euclidean"),       # 13 tiles and, at n_split = 7, 56 waves: most chunks are empty
    (128, 1000, 4, "euclidean"),
    (128, 3, 8, "inner"),
    (960, 3, 8, "euclidean"),
    (960, 1, 4, "inner"),
    (960, 3, 1, "inner"),
]


@pytest.mark.parametrize("d,nq,n_probe,distance", RANGE_CASES)
def test_range_against_the_oracle(d, nq, n_probe, distance):
    """Per-query thresholds from the oracle's own candidate values, then -inf, +inf and NaN; every n_split gives the
    oracle's lims, addresses and value bits, hence the same as every other n_split.  A single query cannot both have
    no hit and have every candidate hit: with nq = 1 the condition on the inputs is met by three runs of the query
    (thresholds on its smallest value, above its largest, on its median) instead of by three queries of one run."""
    case = _range_case(2000 * d + nq + n_probe, d, nq, n_probe)
    args = (case["vectors"], case["query"], case["is_empty"], case["cs"], case["sz"], case["npl"])
    cand = rorc.candidates(*args, _metric(distance))
    n_cand = np.array([int((~np.isnan(v)).sum()) for _, v in cand])
    runs = [_thresholds(cand, r) for r in ((0,) if nq > 1 else (0, 1, 2))]
    want = [rorc.range_scan(*args, thr, _metric(distance), cand=cand) for thr in runs]
    hits = np.stack([np.diff(w[0]) for w in want])
    if nq > 1:
        _assert_not_vacuous(hits[0], n_cand)
    else:
        _assert_not_vacuous(hits[:, 0], np.repeat(n_cand, 3))
        assert 0 < hits[2, 0] < n_cand[0]
    from torchpq_amd.kernels import IVFFlatRangeHip
    op = IVFFlatRangeHip()
    for thr, w in zip(runs, want):
        for n_split in SPLITS:
            lims, v, a, _ = _run(case, thr, distance, n_split, op)
            print(f"d={d} nq={nq} n_split={op.last_n_split}: {len(a)} hits of {n_cand.sum()} candidates")
            _same((lims, v, a), w)
            if n_split is None:   # the wrapper splits a small batch over several workgroups, leaves a large one whole
                assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
            else:
                assert op.last_n_split == n_split
    # one threshold for the batch, a Python float: -inf is every candidate whose value is not NaN, +inf and NaN nothing
    for t, n_split in ((-np.inf, None), (-np.inf, 7), (np.inf, None), (np.nan, 5)):
        got = _run(case, float(t), distance, n_split, op)[:3]
        w = rorc.range_scan(*args, t, _metric(distance), cand=cand)
        _same(got, w)
        assert len(got[2]) == (n_cand.sum() if t == -np.inf else 0)


def test_without_a_tombstone_mask_and_mixed_special_thresholds():
    case = _range_case(77, 24, 6, 8, tomb=0)
    args = (case["vectors"], case["query"], None, case["cs"], case["sz"], case["npl"])
    cand = rorc.candidates(*args)
    thr = _thresholds(cand)
    thr[2], thr[3] = np.nan, -np.inf
    want = rorc.range_scan(*args, thr, cand=cand)
    assert want[0][3] == want[0][2] and want[0][4] - want[0][3] == len(cand[3][0]) > 0
    for n_split in (1, 6):
        _same(_run(case, thr, "euclidean", n_split, with_empty=False)[:3], want)


@pytest.mark.parametrize("n_split", [1, 4])
def test_all_vectors_equal_every_live_probed_slot_in_scan_order(n_split):
    """every slot holds the same vector and the threshold is the common value: all live probed slots, probe rank
    ascending, then address ascending"""
    case = _range_case(5, 24, 3, 8, tomb=40, dup=False)
    case["vectors"][:] = case["vectors"][:, :1]
    case["query"][:] = case["query"][:, :1]
    common = forc.values(case["vectors"], case["query"], np.array([0]))[0, 0]
    lims, v, a, _ = _run(case, float(common), "euclidean", n_split)
    cap = case["vectors"].shape[1]
    slots = [forc.probed_slots(case["cs"][q], case["sz"][q], case["npl"][q], cap) for q in range(3)]
    slots = [s[case["is_empty"][s] == 0] for s in slots]
    assert sum(len(s) for s in slots) > 500 and len(slots[2]) == 0
    assert np.array_equal(lims, np.cumsum([0] + [len(s) for s in slots]))
    assert np.array_equal(a, np.concatenate(slots)) and np.all(v.view(np.uint32) == common.view(np.uint32))
    above = _run(case, float(np.nextafter(common, np.float32(np.inf))), "euclidean", n_split)
    assert len(above[2]) == 0 and not above[0].any()


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_cross_check_with_the_topk_scan(distance):
    """threshold = the k-th value of IVFFlatTopkHip on the same inputs: the range result sorted by (value descending,
    address ascending) starts with exactly the top-k row"""
    from torchpq_amd.kernels import IVFFlatTopkHip
    case = _range_case(31, 24, 7, 8)
    gpu = [T(case[n]) for n in ("vectors", "query", "cs", "sz", "npl")]
    for k in (1, 10, 100):
        tv, ta = IVFFlatTopkHip()(*gpu, k, is_empty=T(case["is_empty"]), distance=distance)
        thr = tv[:, k - 1].contiguous()
        filled = N(ta[:, k - 1] >= 0)
        assert filled.sum() >= 4                      # (-inf pads make the threshold -inf: every candidate)
        lims, v, a, _ = _run(case, N(thr), distance)
        sv, sa = rorc.sort_segments(lims, v, a)
        for q in range(7):
            n = lims[q + 1] - lims[q]
            real = int((N(ta[q]) >= 0).sum())
            assert n >= real and (n >= k if filled[q] else n == real)
            assert np.array_equal(sa[lims[q]:lims[q] + real], N(ta[q])[:real])
            assert np.array_equal(sv[lims[q]:lims[q] + real].view(np.uint32), N(tv[q])[:real].view(np.uint32))


def test_a_nan_query_leaves_the_other_segments_alone():
    case = _range_case(9, 24, 6, 8)
    args = (case["vectors"], case["query"], case["is_empty"], case["cs"], case["sz"], case["npl"])
    thr = _thresholds(rorc.candidates(*args))
    thr[2] = -np.inf
    clean = _run(case, thr, "euclidean", 1)
    assert clean[0][3] > clean[0][2]
    for n_split in (1, 3):
        dirty = dict(case, query=case["query"].copy())
        dirty["query"][5, 2] = np.nan
        lims, v, a, _ = _run(dirty, thr, "euclidean", n_split)
        assert lims[3] == lims[2]                                           # a NaN value is never a hit
        gone = clean[0][3] - clean[0][2]
        assert np.array_equal(np.delete(np.diff(lims), 2), np.delete(np.diff(clean[0]), 2))
        keep = np.r_[0:clean[0][2], clean[0][3]:clean[0][-1]]
        assert len(a) == len(clean[2]) - gone and np.array_equal(a, clean[2][keep])
        assert np.array_equal(v.view(np.uint32), clean[1][keep].view(np.uint32))


def test_fill_never_writes_beyond_a_segment_when_the_inputs_changed():
    """counts from a selective threshold, then a fill pass with -inf (every candidate a hit): each wave stores its
    first wave_count hits and nothing at or beyond the next segment's offset.  The outputs are as long as an unguarded
    fill would need, and hold a canary."""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    case = _range_case(13, 24, 5, 8)
    args = (case["vectors"], case["query"], case["is_empty"], case["cs"], case["sz"], case["npl"])
    cand = rorc.candidates(*args)
    thr = _thresholds(cand, 2)
    n_split, nq, d, n_slots = 3, 5, 24, case["vectors"].shape[1]
    lib = load()
    n_seg = lib.tpq_ivfflat_range_segments(nq, n_split)
    assert n_seg == nq * n_split * 8
    gpu = [T(case[n]) for n in ("vectors", "query", "is_empty", "cs", "sz", "npl")]
    inputs = [ptr(t) for t in gpu]
    shape = (n_slots, d, nq, 8, 0, n_split, stream_ptr(DEV))
    counts = torch.empty(n_seg, device=DEV, dtype=torch.int32)
    t_count, t_fill = T(thr), torch.full((nq,), -np.inf, device=DEV)
    check(lib.tpq_ivfflat_range_count(*inputs, ptr(t_count), ptr(counts), *shape), "count")
    offsets = torch.zeros(n_seg + 1, device=DEV, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    total, n_all = int(offsets[-1]), sum(len(s) for s, _ in cand)
    assert 0 < total < n_all
    vals = torch.full((total + n_all,), 7.5, device=DEV)
    addr = torch.full((total + n_all,), -7, device=DEV, dtype=torch.int64)
    check(lib.tpq_ivfflat_range_fill(*inputs, ptr(t_fill), ptr(offsets), ptr(vals), ptr(addr), *shape), "fill")
    torch.cuda.synchronize()
    assert torch.all(addr[total:] == -7) and torch.all(vals[total:] == 7.5)      # nothing beyond the last segment
    a, off = N(addr[:total]), N(offsets)
    assert np.all(a >= 0)                                                        # every counted place is written
    # each query's places hold candidates of THAT query, in scan order within each wave's segment
    for q in range(nq):
        lo, hi = off[q * n_split * 8], off[(q + 1) * n_split * 8]
        assert np.isin(a[lo:hi], cand[q][0]).all()
    for s in range(n_seg):
        seg = a[off[s]:off[s + 1]]
        assert np.all(np.diff(seg) != 0)


# ---- the index -----------------------------------------------------------------------------------------
def _expected(idx, queries, threshold):
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    _, cells, npl = idx.probe(T(x))
    return rorc.range_search(x, N(idx._storage), N(idx._is_empty), N(idx._cell_start), N(idx._cell_size),
                             N(idx._address2id), N(cells), N(npl), threshold, _metric(idx.distance))


def _check_range_search(idx, queries, threshold):
    thr = T(threshold) if isinstance(threshold, np.ndarray) else threshold
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


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_index_range_search_after_remove_and_expand(distance):
    idx, base, queries, ids, alive = _build(distance, seed=2, nq=20)
    for n_probe, k in ((1, 1), (4, 10), (32, 100)):
        idx.n_probe = n_probe
        thr = _kth_values(idx, queries, k)
        lims, v, i = _check_range_search(idx, queries, thr)
        assert np.all(np.diff(lims)[thr > -1e30] >= k) and lims[-1] > 0
        assert not np.isin(i, ids[~alive]).any()                         # removed ids never come back
    idx.n_probe = 6
    thr = _kth_values(idx, queries, 20)
    before = _check_range_search(idx, queries, thr)
    _check_range_search(idx, queries, float(np.median(thr)))             # one threshold for every query
    # remove what the first query found: its segment empties of them, the others keep theirs
    gone = before[2][before[0][0]:before[0][1]]
    idx.remove(ids=T(gone))
    after = _check_range_search(idx, queries, thr)
    assert not np.isin(after[2], gone).any() and after[0][-1] < before[0][-1]
    idx.expand(torch.arange(0, idx.n_cells, 3, device=DEV))              # addresses move, the hits do not
    moved = _check_range_search(idx, queries, thr)
    assert np.array_equal(moved[0], after[0]) and np.array_equal(moved[2], after[2])
    assert np.array_equal(moved[1].view(np.uint32), after[1].view(np.uint32))
    idx.max_query_batch = 7                                              # 20 queries: batches of 7, 7 and 6
    batched = _check_range_search(idx, queries, thr)
    for got, want in zip(batched, moved):
        assert np.array_equal(got, want)
    idx.max_query_batch = 32768
    empty = idx.range_search(T(queries[:, :0]), -1.0, return_address=True)
    assert empty[0].tolist() == [0] and all(t.numel() == 0 for t in empty[1:]) and len(empty) == 4
    assert empty[1].dtype == torch.float32 and empty[2].dtype == empty[3].dtype == torch.int64


def test_range_search_is_brute_force_with_every_cell_probed_on_integer_data():
    """n_probe = n_cells, integer-valued data (fp32 sums are exact): the hits are float64 brute force over the live
    vectors -- every live vector within the radius, none else"""
    idx, base, queries, ids, alive = _build(integer=True, seed=3)
    idx.n_probe = idx.n_cells
    idx.use_smart_probing = False
    b64, q64 = base[:, alive].astype(np.float64), queries.astype(np.float64)
    live_ids = ids[alive]
    live_adr = N(idx.get_address_by_id(T(live_ids)))
    exact = np.stack([-((q64[:, q:q + 1] - b64) ** 2).sum(0) for q in range(queries.shape[1])])
    assert np.abs(exact).max() < 2 ** 24
    thr = np.sort(exact, axis=1)[:, -30].astype(np.float32)             # ON the 30th best value of each query
    thr[1] = np.float32(exact[1].max() + 1)                             # nothing is that close
    lims, v, i, a = (N(t) for t in idx.range_search(T(queries), T(thr), return_address=True, sort=True))
    _check_range_search(idx, queries, thr)
    assert lims[2] == lims[1] and lims[-1] >= 30 * (queries.shape[1] - 1)
    for q in range(queries.shape[1]):
        keep = np.flatnonzero(exact[q] >= float(thr[q]))
        order = keep[np.lexsort((live_adr[keep], -exact[q][keep]))]
        seg = slice(lims[q], lims[q + 1])
        assert np.array_equal(i[seg], live_ids[order]) and np.array_equal(a[seg], live_adr[order])
        assert np.array_equal(v[seg].astype(np.float64), exact[q][order])
