"""GPU: FlatIndex filtered exact search (tpq_flat_topk_filtered, tpq_flat_range_filtered_count / _fill) against
tests/flat_oracle.py / tests/flat_range_oracle.py handed an id map in which every disallowed slot is -1: ids and
addresses equal, values bit-equal (the fmaf chains are the same, so the tolerance is zero)."""
import numpy as np
import pytest
import torch

import flat_filtered_guarded
import flat_oracle as florc
import flat_range_oracle as frorc
import guarded_alloc
from test_gpu_flat_range import _thresholds
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu


def _metric(distance):
    return "euclidean" if distance == "euclidean" else "inner"


def _allowed(kind, n, rng):
    """one allowed set over n slots, chosen for the gather's edges; an int: exactly that many set bits"""
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "gap":        # some in the first 256-slot chunk, none in the second, some from the third on
        m[rng.choice(256, 40, replace=False)] = True
        m[512 + rng.choice(n - 512, 40, replace=False)] = True
    elif kind == "edges":      # both sides of a word, of a 32-row tile and of a 256-slot boundary
        m[[s for s in (0, 30, 31, 32, 33, 63, 64, 254, 255, 256, 257, 511, 512, n - 1) if s < n]] = True
    elif kind != "none":
        m[rng.choice(n, min(kind, n), replace=False)] = True
    return m


def _pack(masks, n, extra=0):
    """bit rows by hand, int32 [rows, stride]: bit a & 31 of word a >> 5; `extra` words of stride beyond the need,
    and the bits of the last word at and beyond n set (stale bits the kernel must ignore)"""
    stride = (-(-n // 32) + 3) // 4 * 4 + extra
    b = np.zeros((len(masks), stride * 32), bool)
    b[:, :n] = masks
    b[:, n:-(-n // 32) * 32] = True
    return np.packbits(b.reshape(len(masks), stride, 32), axis=-1, bitorder="little").view("<u4")[..., 0].view(np.int32)


def _rows(nq, n_rows, rng):
    """a row per query, shuffled: the first row's run is 100 of 130 queries -- it ends inside a 128-query block and
    inside a 32-query wave -- and one query names a row outside the filter"""
    if nq == 1:
        return np.zeros(1, np.int32)
    at = np.arange(nq)
    rows = np.minimum((at >= nq * 100 // 130).astype(np.int32) + (at >= nq * 127 // 130), n_rows - 1).astype(np.int32)
    rng.shuffle(rows)
    rows[nq // 2] = n_rows + 4
    return rows


def _problem(case):
    d, n, nq, distance, _, _, kinds = case
    rng = np.random.default_rng(1000 * d + n + nq)
    y, x = rng.standard_normal((d, n)).astype(np.float32), rng.standard_normal((d, nq)).astype(np.float32)
    if distance == "cosine":
        y, x = (y / np.linalg.norm(y, axis=0)).astype(np.float32), (x / np.linalg.norm(x, axis=0)).astype(np.float32)
    a2id = rng.permutation(n).astype(np.int64) * 3 + 1
    if n > 1:
        a2id[rng.random(n) < 0.1] = -1
        a2id[[s for s in (31, 256) if s < n]] = -1        # tombstones under set bits of "edges" and "all"
    masks = np.stack([_allowed(kind, n, rng) for kind in kinds])
    rows = _rows(nq, len(kinds), rng)
    fn = florc.values_d1 if d == 1 else florc.values
    vals = (fn(y, x, _metric(distance)) + np.float32(0)).astype(np.float32)
    return y, x, a2id, masks, rows, vals


def _masked(a2id, masks, row):
    return np.where(masks[row], a2id, -1) if 0 <= row < len(masks) else np.full_like(a2id, -1)


def _want_topk(vals, a2id, masks, rows, k):
    out = [florc.topk(vals[q:q + 1], k, _masked(a2id, masks, rows[q])) for q in range(vals.shape[0])]
    return tuple(np.concatenate(t) for t in zip(*out))


def _want_range(vals, thr, a2id, masks, rows):
    hits = [frorc.range_hits(vals[q:q + 1], thr[q], _masked(a2id, masks, rows[q])) for q in range(vals.shape[0])]
    lims = np.concatenate([[0], np.cumsum([h[0][1] for h in hits])]).astype(np.int64)
    return (lims, *(np.concatenate([h[j] for h in hits]) for j in (1, 2, 3)))


def _same(got, want):
    for g, w in zip(got, want):
        g = N(g) if torch.is_tensor(g) else g
        assert g.shape == w.shape and g.dtype == w.dtype
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)) if g.dtype == np.float32 else np.array_equal(g, w)


# (d, n_slots, nq, distance, n_parts, k, the allowed sets of the filter's rows); n_parts = 9 is above the 4 chunks
CASES = [
    (1, 1, 1, "euclidean", None, 1, ("all", "none")),
    (3, 31, 33, "inner", 1, 64, ("all", 1, "none")),
    (17, 257, 129, "cosine", 3, 65, (255, 256, 257)),
    (40, 700, 130, "euclidean", 7, 100, ("gap", "edges", 1)),
    (17, 1000, 130, "inner", None, 100, ("all", 257, "edges")),
    (3, 700, 33, "euclidean", 3, 64, ("gap", "none", 256)),
    (40, 1000, 129, "cosine", 9, 1, ("edges", 255, "all")),
    (1, 1000, 130, "inner", 1, 65, (1, "all", "gap")),
    (3, 20000, 33, "euclidean", 2, 64, ("all", 300, "edges")),   # more than one 8192-slot gather step in a part
]
_IDS = [f"d{c[0]}-n{c[1]}-q{c[2]}-{c[3][:3]}-p{c[4]}-k{c[5]}" for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_topk_against_the_oracle(case):
    from torchpq_amd.kernels import FlatTopkFilteredHip
    d, n, nq, distance, n_parts, k, kinds = case
    y, x, a2id, masks, rows, vals = _problem(case)
    assert n == 1 or (masks & (a2id < 0)).any()          # a tombstone under a set bit
    op = FlatTopkFilteredHip()
    for extra in (0, 4):                                   # the filter's stride larger than needed
        bits = T(_pack(masks, n, extra))
        got = op(T(y), T(x), k, bits, T(rows), address2id=T(a2id), distance=distance, n_parts=n_parts)
        want = _want_topk(vals, a2id, masks, rows, k)
        _same(got, want)
        assert (want[1] < 0).any() or nq == 1             # pads: a row that allows fewer than k, or nothing
    # no rows: every query uses row 0, in groups of 128
    _same(op(T(y), T(x), k, bits, address2id=T(a2id), distance=distance, n_parts=n_parts),
          _want_topk(vals, a2id, masks, np.zeros(nq, np.int32), k))
    assert op.last_n_groups == -(-nq // 128)


@pytest.mark.parametrize("case", CASES, ids=_IDS)
def test_range_against_the_oracle(case):
    from torchpq_amd.kernels import FlatRangeFilteredHip
    d, n, nq, distance, n_parts, _, kinds = case
    y, x, a2id, masks, rows, vals = _problem(case)
    op = FlatRangeFilteredHip()
    bits = T(_pack(masks, n, 4))
    for rotate in ((0,) if nq > 1 else (0, 1, 2)):
        # exactly ON a value of the query's own allowed live slots: the smallest, one ulp above the largest, the median
        thr = np.stack([_thresholds(vals[q:q + 1], _masked(a2id, masks, rows[q]), q + rotate)[0] for q in range(nq)])
        want = _want_range(vals, thr, a2id, masks, rows)
        got = op(T(y), T(x), T(thr), bits, T(rows), address2id=T(a2id), distance=distance, n_parts=n_parts)
        _same(got, want)
    assert want[0][-1] > 0 and (np.diff(want[0]) == 0).any() or nq == 1
    every = op(T(y), T(x), float("-inf"), bits, address2id=T(a2id), distance=distance, n_parts=n_parts)
    _same(every, _want_range(vals, np.full(nq, -np.inf, np.float32), a2id, masks, np.zeros(nq, np.int32)))


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_integer_data_equals_float64_brute_force(distance):
    """components in -8 ... 8, d = 40: every sum is an integer below 2^24, so fp32 is exact in any order"""
    from torchpq_amd.kernels import FlatRangeFilteredHip, FlatTopkFilteredHip
    y, x, a2id = frorc.integer_problem()
    n, nq, k = y.shape[1], x.shape[1], 30
    rng = np.random.default_rng(5)
    masks = np.stack([rng.random(n) < 0.5, rng.random(n) < 0.1])
    rows = (np.arange(nq) % 2).astype(np.int32)
    exact = frorc.exact_values(y, x, distance)
    assert np.abs(exact).max() < 2 ** 24 and 4 * 40 * 8 * 8 < 2 ** 24   # 2 dot - |x|^2 - |y|^2 and every partial sum
    bits = T(_pack(masks, n))
    v, a, i = (N(t) for t in FlatTopkFilteredHip()(T(y), T(x), k, bits, T(rows), address2id=T(a2id), distance=distance))
    thr = np.zeros(nq, np.float32)
    for q in range(nq):
        ok = np.nonzero(masks[rows[q]] & (a2id >= 0))[0]
        order = ok[np.lexsort((ok, -exact[q, ok]))][:k]      # ties (the run of equal vectors) by address
        assert np.array_equal(a[q], order) and np.array_equal(i[q], a2id[order])
        assert np.array_equal(v[q].astype(np.float64), exact[q, order])
        thr[q] = exact[q, order[20]]
    lims, rv, ra, ri = (N(t) for t in FlatRangeFilteredHip()(T(y), T(x), T(thr), bits, T(rows), address2id=T(a2id),
                                                             distance=distance))
    for q in range(nq):
        ok = np.nonzero(masks[rows[q]] & (a2id >= 0))[0]
        keep = ok[exact[q, ok] >= float(thr[q])]
        seg = slice(lims[q], lims[q + 1])
        assert len(keep) >= 21 and np.array_equal(ra[seg], keep) and np.array_equal(ri[seg], a2id[keep])
        assert np.array_equal(rv[seg].astype(np.float64), exact[q, keep])


def _check_index(index, flt, queries, sets, rows, k, thr):
    """search_filtered and range_search_filtered (plain and sorted) against the oracles on the index's own storage"""
    q, storage, a2id = queries, index._storage[:, :, 0], N(index._address2id)
    if index.distance == "cosine":
        q = N(T(queries) / (T(queries).norm(dim=-2, keepdim=True) + 1e-8))
        storage = storage / (storage.norm(dim=-2, keepdim=True) + 1e-8)
    vals = frorc.values(N(storage), q, _metric(index.distance))
    masks = np.stack([np.isin(a2id, s) & (a2id >= 0) for s in sets])
    r = np.zeros(len(q.T), np.int32) if rows is None else rows
    tr = None if rows is None else T(rows)
    v, i, a = index.search_filtered(T(queries), k, flt, tr, return_address=True)
    wv, wa, wi = _want_topk(vals, a2id, masks, r, min(k, index.capacity))
    _same((v, a, i), (wv, wa, wi))
    assert all(torch.equal(s, t) for s, t in zip(index.search_filtered(T(queries), k, flt, tr), (v, i)))
    t = np.full(len(r), thr, np.float32)
    wl, rv, ra, ri = _want_range(vals, t, a2id, masks, r)
    _same(index.range_search_filtered(T(queries), float(thr), flt, tr, return_address=True), (wl, rv, ri, ra))
    sv, sa, si = frorc.sort_segments(wl, rv, ra, ri)
    _same(index.range_search_filtered(T(queries), T(t), flt, tr, return_address=True, sort=True), (wl, sv, si, sa))
    return wi


@pytest.mark.parametrize("distance", ["euclidean", "cosine", "inner"])
def test_index_filters_follow_add_remove_reuse_and_growth(distance):
    from torchpq_amd.index import FlatIndex
    rng = np.random.default_rng(9)
    d, n, nq, k = 24, 1500, 10, 20
    base, queries = rng.standard_normal((d, n)).astype(np.float32), rng.standard_normal((d, nq)).astype(np.float32)
    flat = FlatIndex(d_vector=d, initial_size=1024, device=DEV, distance=distance)
    ids = np.arange(n, dtype=np.int64) * 2 + 5
    sets = [ids[rng.random(n) < 0.5], ids[rng.random(n) < 0.05]]
    flt = flat.id_filter([T(s) for s in sets])          # made before anything is stored
    rows = (np.arange(nq) % 3).astype(np.int32)                        # row 2 is outside the filter
    thr = {"euclidean": -40.0, "cosine": 0.1, "inner": 3.0}[distance]
    assert (_check_index(flat, flt, queries, sets, rows, k, thr) == -1).all()
    flat.add(T(base[:, :900]), ids=T(ids[:900]))
    found = _check_index(flat, flt, queries, sets, rows, k, thr)
    assert (found[0] >= 0).all() and (found[2] == -1).all()
    flat.remove(ids=T(found[0]))                                       # what query 0 found
    assert not np.isin(_check_index(flat, flt, queries, sets, rows, k, thr)[0], found[0]).any()
    flat.add(T(base[:, 900:1000]), ids=T(ids[900:1000]))               # the freed slots are used again
    _check_index(flat, flt, queries, sets, rows, k, thr)
    flat.add(T(base[:, 1000:]), ids=T(ids[1000:]))                     # growth past the initial capacity
    assert flat.capacity > 1024
    _check_index(flat, flt, queries, sets, None, k, thr)
    whole = flat.search_filtered(T(queries), k, flt, T(rows), return_address=True)
    flat.max_query_batch = 3                                           # batches of 3, 3, 3, 1
    _check_index(flat, flt, queries, sets, rows, k, thr)
    assert all(torch.equal(s, t) for s, t in zip(flat.search_filtered(T(queries), k, flt, T(rows),
                                                                      return_address=True), whole))


def test_index_every_id_allowed_is_the_fused_search_and_the_limit_of_1024():
    from torchpq_amd.index import FlatIndex
    rng = np.random.default_rng(2)
    d, n, nq = 17, 3000, 130
    flat = FlatIndex(d_vector=d, initial_size=4096, device=DEV)
    flat.add(T(rng.standard_normal((d, n)).astype(np.float32)))
    flat.remove(ids=T(np.arange(0, n, 7, dtype=np.int64)))
    x = T(rng.standard_normal((d, nq)).astype(np.float32))
    flt = flat.id_filter(torch.arange(n, device=DEV))
    got = flat.search_filtered(x, 100, flt, return_address=True)       # use_fused_search is off: the HIP route anyway
    flat.use_fused_search = True
    want = flat.search(x, 100, return_address=True)
    assert all(torch.equal(g.view(torch.int32), w.view(torch.int32)) for g, w in zip(got, want))
    with pytest.raises(ValueError, match="1024"):
        flat.search_filtered(x, 1025, flt)
    assert flat.search_filtered(x, 1024, flt)[0].shape == (nq, 1024)


def test_filtered_search_inside_guarded_buffers(monkeypatch):
    """the case of tests/flat_filtered_guarded.py with every output and workspace of the wrappers between canaries: the
    guards stay intact, and the results are the same bits from 0x00- and 0xFF-filled buffers -- a merge that read a
    list nobody wrote (a part without an allowed slot, a row that allows nothing) would differ"""
    out = guarded_alloc.run_guarded(flat_filtered_guarded.build(), monkeypatch=monkeypatch)
    for arena in guarded_alloc.run_guarded.arenas.values():
        assert len(arena.allocations) >= 8
    for s, t in zip(out[0x00], out[0xFF]):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.view(torch.uint8), t.view(torch.uint8))
    y, x, a2id, masks, rows, vals = _problem(CASES[3])
    _same(out[0x00][:3], _want_topk(vals, a2id, masks, rows, 100))
    assert out[0x00][3][-1] > 0
