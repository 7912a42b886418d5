"""GPU: FlatIndex range search (tpq_flat_range_count / tpq_flat_range_fill) against tests/flat_range_oracle.py -- lims
equal, addresses and ids equal and in the same order, values bit-equal -- and the index end to end (range_search
across add, remove, slot reuse and growth; batches, sort, cosine; IVFFlatIndex with every cell probed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import flat_oracle as florc
import flat_range_oracle as frorc
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu

PARTS = (None, 1, 2, 5, 7)
# tombstones on both sides of a 4-row group, a 32-slot tile and a 256-slot chunk
EDGE_TOMBS = (2, 3, 4, 5, 30, 31, 32, 33, 254, 255, 256, 257)


def _metric(distance):
    return "euclidean" if distance == "euclidean" else "inner"


def _problem(seed, d, n, nq, distance="euclidean", tombs=True):
    """random stored vectors and queries ("cosine": both of unit length, as the caller of the kernel makes them) and an
    id map with tombstones at EDGE_TOMBS and at a tenth of the other slots; tombs=False: no id map"""
    rng = np.random.default_rng(seed)
    y, x = rng.standard_normal((d, n)).astype(np.float32), rng.standard_normal((d, nq)).astype(np.float32)
    if distance == "cosine":
        y, x = (y / np.linalg.norm(y, axis=0)).astype(np.float32), (x / np.linalg.norm(x, axis=0)).astype(np.float32)
    a2id = None
    if tombs:
        a2id = rng.permutation(n).astype(np.int64) * 3 + 1
        if n > 1:
            a2id[rng.random(n) < 0.1] = -1
            a2id[[s for s in EDGE_TOMBS if s < n]] = -1
    return y, x, a2id


def _thresholds(vals, a2id, rotate=0):
    """per-query thresholds taken from the query's own values over the live slots, so each sits exactly ON a value: by
    turns the smallest (every live slot is a hit), one ulp above the largest (no hit), the median, the upper decile"""
    live = np.ones(vals.shape[1], bool) if a2id is None else a2id >= 0
    thr = np.zeros(vals.shape[0], np.float32)
    for q in range(vals.shape[0]):
        v = np.sort(vals[q][live & ~np.isnan(vals[q])])
        if len(v):
            thr[q] = (v[0], np.nextafter(v[-1], np.float32(np.inf)), v[len(v) // 2], v[(9 * len(v)) // 10])[(q + rotate) % 4]
    return thr


def _run(y, x, thr, a2id, distance, n_parts=None, op=None):
    from torchpq_amd.kernels import FlatRangeHip
    op = op or FlatRangeHip()
    lims, v, a, ids = op(T(y), T(x), T(thr) if isinstance(thr, np.ndarray) else thr,
                         address2id=None if a2id is None else T(a2id), distance=distance, n_parts=n_parts)
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and a.dtype == torch.int64
    assert lims.shape == (x.shape[1] + 1,) and v.shape == a.shape == (int(lims[-1]),)
    assert (ids is None) == (a2id is None)
    if ids is not None:
        assert ids.dtype == torch.int64 and ids.shape == a.shape
    return N(lims), N(v), N(a), None if ids is None else N(ids)


def _same(got, want):
    (lims, v, a, ids), (el, ev, ea, ei) = got, want
    assert np.array_equal(lims, el)
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    assert (ids is None and ei is None) or np.array_equal(ids, ei)


# (d, n_slots, nq, distance, id map): every d, n_slots and nq of the issue, the three distances, with and without a map
CASES = [
    (1, 1, 1, "euclidean", True), (1, 300, 33, "inner", True), (1, 1000, 130, "euclidean", False),
    (3, 31, 1, "inner", True), (3, 257, 129, "euclidean", True), (3, 1000, 33, "cosine", True),
    (17, 1, 33, "inner", False), (17, 31, 130, "euclidean", True), (17, 300, 1, "cosine", True),
    (17, 1000, 129, "inner", True), (40, 257, 33, "cosine", False), (40, 300, 130, "inner", True),
    (40, 1000, 1, "euclidean", True), (40, 31, 129, "cosine", True), (128, 1, 129, "euclidean", True),
    (128, 257, 1, "inner", False), (128, 300, 129, "euclidean", True), (128, 1000, 130, "cosine", True),
    (128, 1000, 33, "euclidean", False), (128, 31, 33, "inner", True),
]


@pytest.mark.parametrize("d,n,nq,distance,tombs", CASES)
def test_range_against_the_oracle(d, n, nq, distance, tombs):
    """Per-query thresholds from the oracle's own values (exact ties; a query without a hit; a query whose every live
    slot is a hit), then -inf, +inf and NaN; every n_parts -- more parts than chunks among them -- gives the oracle's
    lims, addresses, ids and value bits.  A single query cannot both have no hit and have every slot hit: with nq = 1
    three runs of the query (thresholds on its smallest value, above its largest, on its median) stand in."""
    from torchpq_amd.kernels import FlatRangeHip
    y, x, a2id = _problem(1000 * d + n + nq, d, n, nq, distance, tombs)
    vals = frorc.values(y, x, _metric(distance))
    n_live = n if a2id is None else int((a2id >= 0).sum())
    assert n_live > 0
    runs = [_thresholds(vals, a2id, r) for r in ((0,) if nq > 1 else (0, 1, 2))]
    want = [frorc.range_hits(vals, thr, a2id) for thr in runs]
    hits = np.concatenate([np.diff(w[0]) for w in want])
    assert (hits == 0).any() and (hits == n_live).any() and hits.sum() > 0, hits      # the inputs are not vacuous
    op = FlatRangeHip()
    for thr, w in zip(runs, want):
        for n_parts in PARTS:
            got = _run(y, x, thr, a2id, distance, n_parts, op)
            print(f"d={d} n={n} nq={nq} n_parts={op.last_n_parts}: {len(got[2])} hits of {nq * n_live}")
            _same(got, w)
            chunks = -(-n // 256)
            assert op.last_n_parts == (n_parts if n_parts is not None else chunks)   # (small: one chunk per part)
    for t, n_parts in ((-np.inf, None), (-np.inf, 7), (np.inf, None), (np.nan, 5)):
        got = _run(y, x, float(t), a2id, distance, n_parts, op)
        _same(got, frorc.range_hits(vals, t, a2id))
        assert len(got[2]) == (nq * n_live if t == -np.inf else 0)


@pytest.mark.parametrize("n_parts", [1, 4])
def test_all_vectors_equal_every_live_slot_in_address_order(n_parts):
    """every slot holds the same vector and the threshold is below the common value: each query's hits are exactly the
    live addresses, ascending -- the order of the rows, not of the accumulator registers (a tile's rows alternate
    between the half-waves in groups of four)"""
    y, x, a2id = _problem(3, 17, 1000, 33)
    y[:] = y[:, :1]
    x[:] = x[:, :1]
    common = frorc.values(y, x)[0, 0]
    live = np.nonzero(a2id >= 0)[0]
    assert 800 < len(live) < 1000
    lims, v, a, ids = _run(y, x, float(np.nextafter(common, np.float32(-np.inf))), a2id, "euclidean", n_parts)
    assert np.array_equal(lims, np.arange(34) * len(live))
    assert np.array_equal(a, np.tile(live, 33)) and np.array_equal(ids, a2id[a])
    assert np.all(v.view(np.uint32) == common.view(np.uint32))
    on = _run(y, x, float(common), a2id, "euclidean", n_parts)             # ON the value: still every live slot
    assert np.array_equal(on[2], a)
    above = _run(y, x, float(np.nextafter(common, np.float32(np.inf))), a2id, "euclidean", n_parts)
    assert len(above[2]) == 0 and not above[0].any()


@pytest.mark.parametrize("distance", ["inner", "euclidean"])
@pytest.mark.parametrize("tombs", [True, False])
def test_rows_past_the_last_slot_are_never_hits(distance, tombs):
    """n_slots = 300 and threshold -inf: exactly the live slots, none at or beyond 300.  The rows 300 ... 511 of the
    second chunk score -inf for -squared-L2 but 0 for the inner product: only the live mask keeps them out."""
    y, x, a2id = _problem(8, 17, 300, 33, distance, tombs)
    live = np.arange(300) if a2id is None else np.nonzero(a2id >= 0)[0]
    for n_parts in (1, 2, 5):
        lims, v, a, ids = _run(y, x, float(-np.inf), a2id, distance, n_parts)
        assert a.max() < 300 and np.array_equal(lims, np.arange(34) * len(live))
        assert np.array_equal(a, np.tile(live, 33))
        _same((lims, v, a, ids), frorc.range_search(y, x, -np.inf, a2id, distance))
    # a threshold of 0 on inner products: the pad rows' value
    if distance == "inner":
        _same(_run(y, x, 0.0, a2id, distance, 2), frorc.range_search(y, x, 0.0, a2id, distance))


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_special_thresholds_and_values(distance):
    """+inf, -inf and NaN thresholds in one batch; a live stored vector with an inf component (its value is -inf or
    NaN: a hit only at -inf, and only where it is not NaN); a NaN query leaves every other query's segment alone"""
    y, x, a2id = _problem(21, 24, 600, 9, distance)
    a2id[[70, 71]] = [7000, 7100]
    y[3, 70] = np.inf
    y[5, 71] = -np.inf
    x[3, 4] = 0.0                                        # 0 * inf: NaN for query 4, whatever the metric
    vals = frorc.values(y, x, distance)
    assert np.isnan(vals[4, 70]) and not np.isfinite(vals[:, [70, 71]]).any()
    assert np.isneginf(vals[:, [70, 71]]).any()
    thr = _thresholds(vals, a2id)
    thr[0], thr[1], thr[2], thr[4], thr[5] = np.inf, -np.inf, np.nan, -np.inf, -np.inf
    want = frorc.range_hits(vals, thr, a2id)
    hits, n_live = np.diff(want[0]), int((a2id >= 0).sum())
    # (v >= +inf holds for an inner product of +inf; no other value reaches it)
    assert hits[0] == np.isposinf(vals[0][a2id >= 0]).sum() <= 2 and hits[2] == 0 and hits[4] < n_live
    assert hits[1] == (~np.isnan(vals[1][a2id >= 0])).sum()
    assert np.isin([70, 71], want[2][want[0][1]:want[0][2]]).sum() == (~np.isnan(vals[1, [70, 71]])).sum()
    for n_parts in (1, 3):
        _same(_run(y, x, thr, a2id, distance, n_parts), want)
    # a NaN query: its own segment is empty, every other segment is what it is without it
    dirty = x.copy()
    dirty[7, 5] = np.nan
    for n_parts in (1, 3):
        lims, v, a, ids = _run(y, dirty, thr, a2id, distance, n_parts)
        assert lims[6] == lims[5]
        keep = np.r_[0:want[0][5], want[0][6]:want[0][-1]]
        assert np.array_equal(np.delete(np.diff(lims), 5), np.delete(hits, 5))
        assert np.array_equal(a, want[2][keep]) and np.array_equal(ids, want[3][keep])
        assert np.array_equal(v.view(np.uint32), want[1][keep].view(np.uint32))


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_cross_check_with_the_fused_topk(distance):
    """threshold = the 10th value of FlatTopkHip on the same inputs, no tie among the best 11: the hits sorted by (value
    descending, address ascending) are exactly the top-k rows, values bit-equal"""
    from torchpq_amd.kernels import FlatTopkHip
    k = 10
    y, x, a2id = _problem(31, 40, 1000, 33, distance)
    vals = frorc.values(y, x, distance)
    for q in range(33):                                  # the k + 1 best values of every query are distinct
        assert len(np.unique(np.sort(vals[q][a2id >= 0])[-(k + 1):])) == k + 1
    tv, ta, ti = FlatTopkHip()(T(y), T(x), k, address2id=T(a2id), distance=distance)
    lims, v, a, ids = _run(y, x, N(tv[:, k - 1].contiguous()), a2id, distance)
    assert np.array_equal(lims, np.arange(34) * k)
    sv, sa, si = frorc.sort_segments(lims, v, a, ids)
    assert np.array_equal(sa.reshape(33, k), N(ta)) and np.array_equal(si.reshape(33, k), N(ti))
    assert np.array_equal(sv.reshape(33, k).view(np.uint32), N(tv).view(np.uint32))


@pytest.mark.parametrize("with_ids", [True, False])
def test_fill_never_writes_beyond_a_segment_when_the_inputs_changed(with_ids):
    """counts from a selective threshold, then a fill pass with -inf (every live slot a hit): each segment holds the
    first hits of the looser result and nothing is stored at or beyond the next segment's offset.  The outputs are
    surrounded by canaries."""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    d, n, nq, n_parts, pad = 24, 1000, 33, 3, 4096
    y, x, a2id = _problem(13, d, n, nq)
    vals = frorc.values(y, x)
    thr = _thresholds(vals, a2id, 2)
    lib = load()
    n_seg = lib.tpq_flat_range_segments(nq, n_parts)
    assert n_seg == nq * n_parts
    gy, gx, ga = T(y), T(x), T(a2id)
    inputs = (ptr(gy), ptr(gx), ptr(ga))
    shape = (n, d, nq, 0, n_parts, stream_ptr(DEV))
    counts = torch.full((n_seg,), -1, device=DEV, dtype=torch.int32)
    t_count, t_fill = T(thr), torch.full((nq,), -np.inf, device=DEV)
    check(lib.tpq_flat_range_count(*inputs, ptr(t_count), ptr(counts), *shape), "count")
    assert torch.all(counts >= 0) and torch.all(counts.view(nq, n_parts)[:, 2] == 0)   # every segment is written
    offsets = torch.zeros(n_seg + 1, device=DEV, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    total, n_live = int(offsets[-1]), int((a2id >= 0).sum())
    assert np.array_equal(N(offsets)[::n_parts], frorc.range_hits(vals, thr, a2id)[0])
    assert 0 < total < nq * n_live
    out_v = torch.full((pad + total + pad,), 7.5, device=DEV)
    out_a = torch.full((pad + total + pad,), -7, device=DEV, dtype=torch.int64)
    out_i = torch.full((pad + total + pad,), -9, device=DEV, dtype=torch.int64)

    def inner(t):
        return C.c_void_p(t.data_ptr() + pad * t.element_size())
    check(lib.tpq_flat_range_fill(*inputs, ptr(t_fill), ptr(offsets), inner(out_v), inner(out_a),
                                  inner(out_i) if with_ids else None, *shape), "fill")
    torch.cuda.synchronize()
    for t, canary in ((out_v, 7.5), (out_a, -7), (out_i, -9)):
        assert torch.all(t[:pad] == canary) and torch.all(t[pad + total:] == canary)
    if not with_ids:
        assert torch.all(out_i == -9)
    v, a, i, off = N(out_v[pad:pad + total]), N(out_a[pad:pad + total]), N(out_i[pad:pad + total]), N(offsets)
    cpp = -(-(-(-n // 256)) // n_parts) * 256            # slots per part: whole chunks
    live = np.nonzero(a2id >= 0)[0]
    for q in range(nq):
        for p in range(n_parts):
            s = q * n_parts + p
            first = live[(live >= p * cpp) & (live < (p + 1) * cpp)][:off[s + 1] - off[s]]
            assert len(first) == off[s + 1] - off[s]
            assert np.array_equal(a[off[s]:off[s + 1]], first)
            assert np.array_equal(v[off[s]:off[s + 1]].view(np.uint32), vals[q, first].view(np.uint32))
            if with_ids:
                assert np.array_equal(i[off[s]:off[s + 1]], a2id[first])


# ---- the index -----------------------------------------------------------------------------------------
def _expected(index, queries, threshold):
    """the oracle on the index's own storage and id map; for "cosine" queries and stored vectors divided by
    (norm + 1e-8), the normalisation of search()"""
    q, storage = queries, index._storage[:, :, 0]
    if index.distance == "cosine":
        q = N(T(queries) / (T(queries).norm(dim=-2, keepdim=True) + 1e-8))
        storage = storage / (storage.norm(dim=-2, keepdim=True) + 1e-8)
    lims, v, a, ids = frorc.range_search(N(storage), q, threshold, N(index._address2id), _metric(index.distance))
    return lims, v, ids, a


def _check_range_search(index, queries, threshold):
    thr = T(threshold) if isinstance(threshold, np.ndarray) else threshold
    lims, v, i, a = index.range_search(T(queries), thr, return_address=True)
    el, ev, ei, ea = _expected(index, queries, threshold)
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and i.dtype == a.dtype == torch.int64
    _same((N(lims), N(v), N(a), N(i)), (el, ev, ea, ei))
    assert np.all(ei >= 0)
    l2, v2, i2 = index.range_search(T(queries), thr)                       # without the addresses
    assert torch.equal(l2, lims) and torch.equal(v2, v) and torch.equal(i2, i)
    ls, vs, is_, as_ = index.range_search(T(queries), thr, return_address=True, sort=True)
    sv, sa, si = frorc.sort_segments(el, ev, ea, ei)
    _same((N(ls), N(vs), N(as_), N(is_)), (el, sv, sa, si))
    return N(lims), N(v), N(i), N(a)


def _kth_values(index, queries, k):
    """per-query thresholds: the k-th value of the fused search -- at least k hits per query"""
    index.use_fused_search = True
    v = N(index.search(T(queries), k=k)[0])[:, k - 1]
    index.use_fused_search = False
    assert np.isfinite(v).all()
    return v.astype(np.float32)


@pytest.mark.parametrize("distance", ["euclidean", "cosine", "inner"])
def test_index_range_search_through_the_index_life_cycle(distance):
    from torchpq_amd.index import FlatIndex
    rng = np.random.default_rng(9)
    d, n, nq, k = 24, 1500, 10, 20
    base, queries = rng.standard_normal((d, n)).astype(np.float32), rng.standard_normal((d, nq)).astype(np.float32)
    base *= np.exp(rng.uniform(np.log(0.2), np.log(5.0), n)).astype(np.float32)     # the distances rank differently
    flat = FlatIndex(d_vector=d, initial_size=1024, device=DEV, distance=distance)
    # an empty index (capacity, no items) and no queries
    for got in (flat.range_search(T(queries), -1e30, return_address=True),
                flat.range_search(T(queries[:, :0]), -1.0, return_address=True, sort=True)):
        assert len(got) == 4 and not got[0].any() and all(t.numel() == 0 for t in got[1:])
        assert got[1].dtype == torch.float32 and got[2].dtype == got[3].dtype == got[0].dtype == torch.int64
    assert flat.range_search(T(queries), -1e30)[0].shape == (nq + 1,)
    ids = torch.arange(n, device=DEV) * 2 + 5
    flat.add(T(base[:, :900]), ids=ids[:900])
    assert flat.capacity == 1024
    thr = _kth_values(flat, queries, k)
    lims, v, i, a = _check_range_search(flat, queries, thr)
    assert np.all(np.diff(lims) >= k) and np.array_equal(i, a * 2 + 5)
    none = flat.range_search(T(queries), float("inf"))
    assert not none[0].any() and none[1].numel() == 0
    _check_range_search(flat, queries, float(np.median(thr)))            # one threshold for every query
    # remove what the first query found: its segment empties of them; add: the freed slots are used again
    gone, gone_at = i[lims[0]:lims[1]], a[lims[0]:lims[1]]
    flat.remove(ids=T(gone))
    after = _check_range_search(flat, queries, thr)
    assert not np.isin(after[2], gone).any() and after[0][-1] < lims[-1]
    _, addr = flat.add(T(base[:, 900:1000]), ids=ids[900:1000], return_address=True)
    assert np.isin(gone_at, N(addr)).all()
    _check_range_search(flat, queries, thr)
    flat.add(T(base[:, 1000:]), ids=ids[1000:])                          # growth past the initial capacity
    assert flat.capacity > 1024
    thr = _kth_values(flat, queries, k)
    whole = _check_range_search(flat, queries, thr)
    assert whole[3].max() >= 1024
    # batches of max_query_batch (3, 3, 3, 1) give the same result as one batch, sorted or not
    whole_sorted = flat.range_search(T(queries), T(thr), return_address=True, sort=True)
    flat.max_query_batch = 3
    batched = _check_range_search(flat, queries, thr)
    for got, want in zip(batched, whole):
        assert np.array_equal(got, want)
    assert all(torch.equal(x, y) for x, y in zip(flat.range_search(T(queries), T(thr), return_address=True, sort=True),
                                                 whole_sorted))
    del flat.max_query_batch
    # it is the HIP route whatever use_fused_search says
    flat.use_fused_search = True
    assert all(torch.equal(x, y) for x, y in zip(flat.range_search(T(queries), T(thr), return_address=True),
                                                 (T(t) for t in whole)))


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_integer_data_equals_brute_force_and_ivfflat_with_every_cell_probed(distance):
    """the integer data of the CPU test (fp32 sums are exact in any order): FlatIndex.range_search equals float64 brute
    force, and IVFFlatIndex.range_search with every cell probed returns the same ids and values for every query
    (IVFFlatIndex has no "inner")"""
    from torchpq_amd.index import FlatIndex, IVFFlatIndex
    y, x, a2id = frorc.integer_problem()
    live = np.nonzero(a2id >= 0)[0]
    flat = FlatIndex(d_vector=y.shape[0], initial_size=y.shape[1], device=DEV, distance=distance)
    flat.add(T(y), ids=T(np.where(a2id >= 0, a2id, 10 ** 6 + np.arange(len(a2id)))))
    flat.remove(ids=T(10 ** 6 + np.nonzero(a2id < 0)[0]))
    assert np.array_equal(N(flat._address2id), a2id)
    exact = frorc.exact_values(y, x, _metric(distance))
    thr = np.sort(exact[:, live], axis=1)[:, -30].astype(np.float32)     # ON the 30th best value of each query
    thr[1] = np.float32(exact[1].max() + 1)                              # nothing is that close
    thr[2] = np.float32(exact[2, 40])                                    # the 31 equal vectors tie with it
    lims, v, i, a = (N(t) for t in flat.range_search(T(x), T(thr), return_address=True))
    assert lims[2] == lims[1] and lims[-1] >= 30 * (x.shape[1] - 1)
    for q in range(x.shape[1]):
        keep = live[exact[q, live] >= float(thr[q])]
        seg = slice(lims[q], lims[q + 1])
        assert np.array_equal(a[seg], keep) and np.array_equal(i[seg], a2id[keep])
        assert np.array_equal(v[seg].astype(np.float64), exact[q, keep])
    if distance != "euclidean":
        return
    np.random.seed(0)
    torch.manual_seed(0)
    ivf = IVFFlatIndex(y.shape[0], n_cells=8, initial_size=16, distance=distance, device=DEV)
    ivf.train(T(y))
    ivf.add(T(y[:, live]), ids=T(a2id[live]))
    ivf.n_probe = ivf.n_cells
    ivf.use_smart_probing = False
    il, iv, ii = (N(t) for t in ivf.range_search(T(x), T(thr)))
    assert np.array_equal(il, lims)
    for q in range(x.shape[1]):
        seg = slice(lims[q], lims[q + 1])
        order, mine = np.argsort(ii[seg], kind="stable"), np.argsort(i[seg], kind="stable")
        assert np.array_equal(ii[seg][order], i[seg][mine])
        assert np.array_equal(iv[seg][order].astype(np.float64), v[seg][mine].astype(np.float64))
