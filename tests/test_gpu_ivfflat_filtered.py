"""GPU: IVFFlatIndex filtered search.  The masked form of the list scan (tpq_ivfflat_scan_topk with `is_empty` a filter
row OR-ed with the tombstones) against tests/ivfflat_filtered_oracle.py -- addresses equal, value bits equal -- on the
inputs of tests/ivfflat_filtered_cases.py (whose conditions tests/test_ivfflat_filtered_cpu.py asserts), and the index end
to end: search_filtered, search_cells_filtered, range_search_filtered, one guarded run."""
import numpy as np
import pytest
import torch

import guarded_alloc
import ivfflat_filtered_cases as cases
import ivfflat_filtered_oracle as ffo
from test_gpu_ivfflat import _build
from test_gpu_ivfflat_range import _thresholds
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu


def _gpu(case):
    """the case's arrays on the GPU, uploaded once"""
    if "gpu" not in case:
        case["gpu"] = {n: T(case[n]) for n in ("vectors", "query", "cs", "sz", "npl", "masks")}
    return case["gpu"]


@pytest.mark.parametrize("d,nq,n_probe,distance,long", cases.KERNEL_CASES)
def test_masked_scan_against_the_oracle(d, nq, n_probe, distance, long):
    """every mask row, every k and every n_split give the oracle's addresses and value bits, hence the same as every
    other split"""
    from torchpq_amd.kernels import IVFFlatTopkHip
    case = cases.kernel_case(d, nq, n_probe, distance, long)
    g = _gpu(case)
    op = IVFFlatTopkHip()
    for r, row in enumerate(cases.ROWS):
        for k in cases.KS:
            ev, ea = case["want"][r, k]
            for n_split in cases.SPLITS:
                v, a = op(g["vectors"], g["query"], g["cs"], g["sz"], g["npl"], k, is_empty=g["masks"][r],
                          distance=distance, n_split=n_split)
                assert v.shape == a.shape == (nq, k) and v.dtype == torch.float32 and a.dtype == torch.int64
                assert np.array_equal(N(a), ea), (row, k, n_split)
                assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32)), (row, k, n_split)
                if n_split is None:   # the wrapper splits a small batch over several workgroups, leaves a large one whole
                    assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
                else:
                    assert op.last_n_split == n_split
        filled = (case["want"][r, 1024][1] >= 0).sum(1)
        print(f"d={d} nq={nq} {row}: candidates per query min {filled.min()} max {filled.max()}")


# ---- the index -----------------------------------------------------------------------------------------
def _prepared(idx, queries):
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    return x


def _state(idx):
    return (N(idx._storage), N(idx._is_empty), N(idx._cell_start), N(idx._cell_size), N(idx._address2id))


def _expected(idx, queries, id_sets, rows, k):
    """tests/ivfflat_filtered_oracle.search_filtered on the index's own state and the cells its coarse step returns"""
    x = _prepared(idx, queries)
    _, cells, npl = idx.probe(T(x))
    return ffo.search_filtered(x, *_state(idx), N(cells), N(npl), id_sets, rows, k, cases.metric(idx.distance))


def _check(idx, queries, flt, id_sets, rows, k):
    v, i = idx.search_filtered(T(queries), k, flt, None if rows is None else T(rows))
    ev, ei, ea = _expected(idx, queries, id_sets, rows, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and v.shape == i.shape == (queries.shape[1], k)
    assert np.array_equal(N(i), ei)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    return N(v), N(i)


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_index_search_filtered(distance):
    idx, base, queries, ids, alive = _build(distance, seed=2, nq=24)
    removed = np.flatnonzero(~alive)
    nq = queries.shape[1]
    rng = np.random.default_rng(5)
    idx.n_probe = 6
    # one shared set: a tenth of the ids, removed ones and ids the index never held among them
    tenth = np.concatenate([rng.choice(ids, len(ids) // 10, replace=False), ids[removed[:5]], [-3, 4, 10 ** 9]])
    tenth = tenth.astype(np.int64)
    flt = idx.id_filter(T(tenth))
    v, i = _check(idx, queries, flt, [tenth], None, 10)
    found = i[i >= 0]
    assert len(found) and np.isin(found, tenth).all() and not np.isin(found, ids[removed]).any()
    plain_v, plain_i = idx.search(T(queries), k=10)
    assert not np.array_equal(N(plain_i), i)                               # the filter does change the answer
    v, i = _check(idx, queries, flt, [tenth], None, 300)                   # more than most queries can fill
    assert ((i >= 0).sum(1) < 300).sum() > nq // 2
    # per-query rows: everything, one id, nothing, a half
    half = ids[rng.random(len(ids)) < 0.5]
    one = ids[alive][1234:1235]
    sets = [ids, one, np.zeros(0, np.int64), half]
    multi = idx.id_filter([T(s) for s in sets])
    rows = (np.arange(nq) % 4).astype(np.int32)
    v, i = _check(idx, queries, multi, sets, rows, 20)
    sv, si = idx.search(T(queries), k=20)
    assert np.array_equal(i[rows == 0], N(si)[rows == 0])                  # every id allowed: search
    assert np.array_equal(v[rows == 0].view(np.uint32), N(sv)[rows == 0].view(np.uint32))
    assert np.all(i[rows == 2] == -1) and np.all(np.isneginf(v[rows == 2]))           # an empty id set: all padding
    assert np.all(i[rows == 1][:, 1:] == -1) and set(i[rows == 1][:, 0]) <= {-1, int(one[0])}
    v64, i64 = idx.search_filtered(T(queries), 20, multi, T(rows.astype(np.int64)))   # any int tensor chooses the rows
    assert np.array_equal(N(i64), i)
    # rows outside [0, n_filters) give all pads -- with several rows, and with one (where nothing is read back)
    wild = rows.copy()
    wild[::5], wild[1::5] = -1, 4
    v, i = _check(idx, queries, multi, sets, wild, 20)
    assert np.all(i[(wild < 0) | (wild > 3)] == -1)
    single = np.zeros(nq, np.int32)
    single[::3] = 1
    v, i = _check(idx, queries, flt, [tenth], single, 10)
    assert np.all(i[single == 1] == -1) and np.all(np.isneginf(v[single == 1])) and (i[single == 0] >= 0).any()
    every = np.full(nq, 3, np.int32)                                       # one row for the whole batch: one launch
    _check(idx, queries, multi, sets, every, 20)
    empty = idx.id_filter(torch.zeros(0, dtype=torch.int64))
    v, i = _check(idx, queries, empty, [np.zeros(0, np.int64)], None, 5)
    assert np.all(i == -1) and np.all(np.isneginf(v))
    # a filter made before an add that grows the container gives what one made after gives
    cap_before = idx.capacity
    extra = (base[:, :1500] + 0.01).astype(np.float32)
    new_ids = torch.arange(1500, device=DEV) + 100000
    early = [np.concatenate([half, N(new_ids[::3])]), ids[::7]]
    before = idx.id_filter([T(s) for s in early])
    before.masks()                                                         # built for the old addresses
    idx.add(T(extra), ids=new_ids)
    assert idx.capacity > cap_before
    rows2 = (np.arange(nq) % 2).astype(np.int32)
    got_before = _check(idx, queries, before, early, rows2, 50)
    got_after = _check(idx, queries, idx.id_filter([T(s) for s in early]), early, rows2, 50)
    assert np.array_equal(got_before[1], got_after[1]) and np.isin(got_before[1], N(new_ids)).any()
    assert np.array_equal(got_before[0].view(np.uint32), got_after[0].view(np.uint32))
    # ... and follows a remove
    gone = got_before[1][0][got_before[1][0] >= 0][:5]
    idx.remove(ids=T(gone))
    after_remove = _check(idx, queries, before, early, rows2, 50)
    assert not np.isin(after_remove[1], gone).any()
    # a batch larger than max_query_batch equals the unbatched call: the rows are cut alongside the queries
    idx.max_query_batch = 7
    batched = _check(idx, queries, before, early, rows2, 50)
    idx.max_query_batch = 32768
    assert np.array_equal(batched[1], after_remove[1])
    assert np.array_equal(batched[0].view(np.uint32), after_remove[0].view(np.uint32))
    # search_cells_filtered hands back the addresses too
    x = idx._prepare(T(queries))
    sims, cells, npl = idx.probe(x)
    cv, ci, ca = idx.search_cells_filtered(x, cells, before, T(rows2), n_probe_list=npl, k=50, return_address=True)
    assert np.array_equal(N(ci), after_remove[1]) and torch.equal(idx.get_id_by_address(ca)[ca >= 0], ci[ca >= 0])
    assert torch.all((ca >= 0) == (ci >= 0))
    none = idx.search_filtered(T(queries[:, :0]), 5, before)
    assert none[0].shape == none[1].shape == (0, 5)
    none = idx.search_filtered(T(queries[:, :0]), 5, before, torch.zeros(0, device=DEV, dtype=torch.int32))
    assert none[0].shape == none[1].shape == (0, 5)


def _range_expected(idx, queries, id_sets, rows, threshold):
    x = _prepared(idx, queries)
    _, cells, npl = idx.probe(T(x))
    return ffo.range_filtered(x, *_state(idx), N(cells), N(npl), id_sets, rows, threshold, cases.metric(idx.distance))


def _range_thresholds(idx, queries, id_sets, rows):
    """per-query thresholds sitting on the query's own candidate values (test_gpu_ivfflat_range._thresholds)"""
    x = _prepared(idx, queries)
    _, cells, npl = idx.probe(T(x))
    storage, is_empty, cell_start, cell_size, a2i = _state(idx)
    cells = N(cells)
    cand = ffo.candidates(ffo.forc.as_vectors(storage), x, is_empty, ffo.allowed_rows(a2i, id_sets), rows,
                          cell_start[cells], cell_size[cells], N(npl), cases.metric(idx.distance))
    return _thresholds(cand)


def _check_range(idx, queries, flt, id_sets, rows, threshold):
    thr = T(threshold) if isinstance(threshold, np.ndarray) else threshold
    fq = None if rows is None else T(rows)
    lims, v, i, a = idx.range_search_filtered(T(queries), thr, flt, fq, return_address=True)
    el, ev, ei, ea = _range_expected(idx, queries, id_sets, rows, threshold)
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and i.dtype == a.dtype == torch.int64
    assert np.array_equal(N(lims), el) and np.array_equal(N(a), ea) and np.array_equal(N(i), ei)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    l2, v2, i2 = idx.range_search_filtered(T(queries), thr, flt, fq)
    assert torch.equal(l2, lims) and torch.equal(v2, v) and torch.equal(i2, i)
    ls, vs, is_, as_ = idx.range_search_filtered(T(queries), thr, flt, fq, return_address=True, sort=True)
    sv, sa, si = ffo.rorc.sort_segments(el, ev, ea, ei)
    assert np.array_equal(N(ls), el) and np.array_equal(N(as_), sa) and np.array_equal(N(is_), si)
    assert np.array_equal(N(vs).view(np.uint32), sv.view(np.uint32))
    return el, ev, ei


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_index_range_search_filtered(distance):
    idx, base, queries, ids, alive = _build(distance, seed=4, nq=20)
    nq = queries.shape[1]
    rng = np.random.default_rng(9)
    idx.n_probe = 6
    half = ids[rng.random(len(ids)) < 0.5]
    tenth = np.concatenate([rng.choice(ids, len(ids) // 10, replace=False), ids[~alive][:5], [-3, 10 ** 9]]).astype(np.int64)
    # one row, no filter_of_query
    flt = idx.id_filter(T(tenth))
    thr = _range_thresholds(idx, queries, [tenth], None)
    lims, v, i = _check_range(idx, queries, flt, [tenth], None, thr)
    assert lims[-1] > 0 and np.isin(i, tenth).all() and not np.isin(i, ids[~alive]).any()
    assert (np.diff(lims) == 0).any()                                      # a threshold above the largest value
    _check_range(idx, queries, flt, [tenth], None, float(np.median(thr)))  # one threshold for every query
    # four rows cycled, rows outside the filter among them
    sets = [ids, ids[alive][77:78], np.zeros(0, np.int64), half]
    multi = idx.id_filter([T(s) for s in sets])
    rows = (np.arange(nq) % 4).astype(np.int32)
    rows[9], rows[14] = -1, 4
    thr = _range_thresholds(idx, queries, sets, rows)
    lims, v, i = _check_range(idx, queries, multi, sets, rows, thr)
    hits = np.diff(lims)
    assert hits[rows == 0].sum() > 0 and hits[rows == 3].sum() > 0 and not hits[(rows == 2) | (rows < 0) | (rows > 3)].any()
    _check_range(idx, queries, multi, sets, rows, float(np.median(thr[rows == 3])))
    # the all-ids rows are the unfiltered range search; range_search is what it was
    plain = idx.range_search(T(queries), T(thr), return_address=True)
    every = idx.range_search_filtered(T(queries), T(thr), multi, torch.zeros(nq, device=DEV, dtype=torch.int64),
                                      return_address=True)
    for got, want in zip(every, plain):
        assert torch.equal(got, want)
    from test_gpu_ivfflat_range import _check_range_search
    _check_range_search(idx, queries, thr)
    # batches: the rows and the thresholds are cut alongside the queries
    idx.max_query_batch = 7
    batched = _check_range(idx, queries, multi, sets, rows, thr)
    idx.max_query_batch = 32768
    assert np.array_equal(batched[0], lims) and np.array_equal(batched[2], i)
    empty = idx.range_search_filtered(T(queries[:, :0]), -1.0, multi, return_address=True)
    assert empty[0].tolist() == [0] and all(t.numel() == 0 for t in empty[1:]) and len(empty) == 4


def test_filtered_search_is_brute_force_over_the_allowed_ids_with_every_cell_probed():
    """n_probe = n_cells, integer-valued data (fp32 sums are exact): the filtered result is float64 brute force over
    the live vectors whose id the filter allows, equal values by slot address"""
    idx, base, queries, ids, alive = _build(integer=True, seed=3)
    idx.n_probe = idx.n_cells
    idx.use_smart_probing = False
    k = 50
    rng = np.random.default_rng(2)
    sets = [ids[rng.random(len(ids)) < 0.03], ids[rng.random(len(ids)) < 0.5]]
    rows = (np.arange(queries.shape[1]) % 2).astype(np.int32)
    v, i = _check(idx, queries, idx.id_filter([T(s) for s in sets]), sets, rows, k)
    b64, q64 = base.astype(np.float64), queries.astype(np.float64)
    adr = N(idx.get_address_by_id(T(ids)))
    short = 0
    for q in range(queries.shape[1]):
        ok = np.flatnonzero(alive & np.isin(ids, sets[rows[q]]))
        diff = q64[:, q:q + 1] - b64[:, ok]
        exact = -(diff * diff).sum(0)
        assert np.abs(exact).max() < 2 ** 24
        order = np.lexsort((adr[ok], -exact))[:k]
        n = len(order)
        short += n < k
        assert np.array_equal(i[q, :n], ids[ok][order]) and np.all(i[q, n:] == -1)
        assert np.array_equal(v[q, :n].astype(np.float64), exact[order])
    print(f"{short} of {queries.shape[1]} queries have fewer than {k} allowed vectors")


def test_filtered_search_inside_guarded_buffers(monkeypatch):
    """search_filtered and range_search_filtered with every output and workspace of the wrappers between canaries:
    the guards stay intact and the results are identical whether the buffers start as 0x00 or as 0xFF"""
    idx, base, queries, ids, alive = _build("euclidean", seed=6, nq=12)
    idx.n_probe = 5
    rng = np.random.default_rng(1)
    sets = [ids[rng.random(len(ids)) < 0.5], ids[rng.random(len(ids)) < 0.03]]
    flt = idx.id_filter([T(s) for s in sets])
    rows = T((np.arange(12) % 2).astype(np.int32))
    thr = idx.search_filtered(T(queries), 5, flt, rows)[0][:, -1].clamp(min=-1e30).contiguous()

    def run():
        a = idx.search_filtered(T(queries), 100, flt, rows)
        b = idx.range_search_filtered(T(queries), thr, flt, rows, return_address=True)
        return [t.clone() for t in (*a, *b)]

    out = guarded_alloc.run_guarded(run, monkeypatch=monkeypatch)
    for arena in guarded_alloc.run_guarded.arenas.values():
        assert len(arena.allocations) >= 6
    for x, y in zip(out[0x00], out[0xFF]):
        assert x.dtype == y.dtype and x.shape == y.shape
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8))
    assert (out[0x00][1] >= 0).any() and out[0x00][2][-1] > 0
    ev, ei, _ = _expected(idx, queries, sets, N(rows), 100)
    assert np.array_equal(N(out[0x00][1]), ei) and np.array_equal(N(out[0x00][0]).view(np.uint32), ev.view(np.uint32))
