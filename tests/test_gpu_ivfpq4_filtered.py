"""GPU: IVFPQ4Index filtered search (tpq_ivfpq4_scan_filtered_topk / _residual_topk, csrc/scan_pq4_filtered.hip) against
tests/ivfpq4_filtered_oracle.py -- values compared as uint32, addresses equal -- on the inputs of
tests/ivfpq4_filtered_cases.py (whose conditions tests/test_ivfpq4_filtered_cpu.py asserts), against the unfiltered
4-bit scans where the two must agree, and the index end to end."""
import numpy as np
import pytest
import torch

import guarded_alloc
import ivfpq4_cases as pcases
import ivfpq4_filtered_cases as cases
import ivfpq4_filtered_guarded as guarded
import ivfpq4_filtered_oracle as forc
import ivfpq4_residual_cases as rcases
import ivfpq4_residual_oracle as rorc
import ivfpq_filtered_cases as fcases
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _gpu(c):
    """the case's arrays on the GPU, uploaded once"""
    if "gpu" not in c:
        g = {k: T(v) for k, v in c.items() if isinstance(v, np.ndarray) and k not in ("allowed", "bits")}
        g["bits"] = T(c["bits"].view(np.int32))
        c["gpu"] = g
    return c["gpu"]


def _run(c, residual, rows, k, distance, n_split=None, op=None, with_empty=True, bits=None):
    from torchpq_amd.kernels import IVFPQ4FilteredTopkHip
    g = _gpu(c)
    op = op or IVFPQ4FilteredTopkHip(m=c["codebook"].shape[0])
    rows = None if rows is None else (rows if torch.is_tensor(rows) else T(np.asarray(rows, np.int32)))
    kw = dict(filter_of_query=rows, is_empty=g["is_empty"] if with_empty else None, distance=distance, n_split=n_split)
    bits = g["bits"] if bits is None else bits
    if residual:
        v, a = op.residual(g["storage"], g["query"], g["codebook"], g["centroids"], g["cells"], g["cs"], g["sz"],
                           g["npl"], k, bits, **kw)
    else:
        v, a = op(g["storage"], g["query"], g["codebook"], g["cs"], g["sz"], g["npl"], k, bits, **kw)
    assert v.dtype == torch.float32 and a.dtype == torch.int64 and v.shape == a.shape == (c["query"].shape[1], k)
    return N(v), N(a), op


def _same(got, want):
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))


def _oracle(c, residual, rows, k, distance, with_empty=True):
    extra = dict(centroids=c["centroids"], cells=c["cells"]) if residual else {}
    return forc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"] if with_empty else None, c["allowed"],
                          rows, c["cs"], c["sz"], c["npl"], k, distance, **extra)


# ---- 1. the kernels against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", cases.KERNEL_CASES)
def test_scan_against_the_oracle(m, ds, nq, n_probe, distance, residual):
    """every run of filter rows (the last passes no filter_of_query), every k and every n_split give the oracle's
    addresses and value bits, hence the same as every other split"""
    from torchpq_amd.kernels import IVFPQ4FilteredTopkHip
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    op = IVFPQ4FilteredTopkHip(m=m)
    for run, rows in enumerate(c["runs"]):
        for k in cases.KS:
            for n_split in (cases.SPLITS if nq <= 3 else (None,)):
                v, a, _ = _run(c, residual, rows, k, distance, n_split, op)
                _same((v, a), cases.want(c, run, k))
                if n_split is None:   # the wrapper splits a small batch over several workgroups, leaves a large one whole
                    assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
                else:
                    assert op.last_n_split == n_split
                assert np.all(v[a < 0] == -np.inf) and np.all(v[:, 1:] <= v[:, :-1])


# ---- 2. the all-ones row is the unfiltered scan ---------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_all_ones_row_is_the_unfiltered_scan_bit_for_bit(distance, residual):
    from torchpq_amd.kernels import IVFPQ4ResidualTopkHip, IVFPQ4TopkHip
    c = cases.case(24, 2, 3, 4, "euclidean", residual)
    g = _gpu(c)
    for n_split in (1, 3):
        for k in (10, 100):
            if residual:
                ev, ea = IVFPQ4ResidualTopkHip(m=24)(g["storage"], g["query"], g["codebook"], g["centroids"],
                                                     g["cells"], g["cs"], g["sz"], g["npl"], k, is_empty=g["is_empty"],
                                                     distance=distance, n_split=n_split)
            else:
                ev, ea = IVFPQ4TopkHip(m=24)(g["storage"], g["query"], g["codebook"], g["cs"], g["sz"], g["npl"], k,
                                             is_empty=g["is_empty"], distance=distance, n_split=n_split)
            for rows in (None, np.zeros(3, np.int32)):
                v, a, _ = _run(c, residual, rows, k, distance, n_split)
                _same((v, a), (N(ev), N(ea)))
            assert (N(ea) >= 0).any()


# ---- 3. mixed tables in one batch -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n_split", [1, 4, 7])
def test_every_pending_slot_is_looked_up_in_its_own_probes_table(n_split):
    """every slot holds the same code, so a value depends on the probe's centroid alone, and the filter allows 8 to 12
    live slots per cell: the slots a wave values together come from several probes of one group of tables.  A lane
    that looks its slot up in another probe's table gives another cell's value -- which fails here and nowhere else.
    Row 1 allows only tiles 0 and 4 of the 300-slot cell: with n_split = 7 a part begins inside that cell."""
    c = cases.mixed_table_case()
    cap = c["storage"].shape[1]
    for row in (0, 1):
        rows = np.full(3, row, np.int32)
        for k in (1, 10, 100):
            v, a, _ = _run(c, True, rows, k, "euclidean", n_split)
            _same((v, a), _oracle(c, True, rows, k, "euclidean"))
            for q in range(3):
                got = a[q][a[q] >= 0]
                if len(got) == 0:
                    continue
                cell_of = {}
                for p, s in zip(*rorc.probe_slots(c["cs"][q], c["sz"][q], c["npl"][q], cap)):
                    cell_of[int(s)] = int(c["cells"][q, p])
                by_cell = np.array([cell_of[int(s)] for s in got])
                vq = v[q][:len(got)]
                for cell in np.unique(by_cell):
                    assert len(np.unique(vq[by_cell == cell])) == 1                  # one value per cell
                    assert np.all(np.diff(got[by_cell == cell]) > 0)                 # addresses ascend within it
        if row == 0:
            # (and the cells' values differ: a wave's two tiles, valued in one batch, lie in different cells)
            assert len(np.unique(v[0][a[0] >= 0])) >= 3
        else:
            big = c["big_start"]
            hit = a[a >= 0]
            assert len(hit) and np.all((hit >= big) & (hit < big + 300))
            assert np.all((hit < big + 64) | (hit >= big + 256))


# ---- 4. a group without an allowed slot between two groups with hits -----------------------------------------------
def _groups(c, q, G):
    """the groups of tables scan_pq4_filtered_residual_kernel walks for query q when it is one workgroup: the probes
    with a tile, G consecutive probes from the first of them, the next group from the next probe with a tile"""
    n = int(min(max(int(c["npl"][q]), 0), c["cs"].shape[1]))
    scanned = [p for p in range(n) if c["sz"][q, p] > 0 and not (p > 0 and c["cs"][q, p] == c["cs"][q, p - 1])]
    groups = []
    while scanned:
        g0 = scanned[0]
        groups.append([p for p in scanned if p < g0 + G])
        scanned = [p for p in scanned if p >= g0 + G]
    return groups


@pytest.mark.parametrize("n_split", [1, 5])
def test_a_group_without_an_allowed_slot_between_two_groups_with_hits(n_split):
    """m = 256: two tables per buffer.  Every query gets a row of its own that allows everything but the cells of its
    second group of probes: that group's walk appends nothing, drains nothing and must still take its barrier"""
    c = dict(cases.case(256, 1, 3, 8, "euclidean", True))
    c.pop("gpu", None)
    cap = c["storage"].shape[1]
    allowed = np.ones((3, cap), bool)
    checked = 0
    for q in range(3):
        groups = _groups(c, q, 2)
        if len(groups) < 3:
            allowed[q] = False                          # (a query of few probes: no candidate at all)
            continue
        for p in groups[1]:
            allowed[q, c["cs"][q, p]:c["cs"][q, p] + c["sz"][q, p]] = False
        checked += 1
    assert checked >= 1
    c["allowed"], c["bits"] = allowed, fcases.filter_bits(allowed)
    rows = np.arange(3, dtype=np.int32)
    for k in (10, 1024):
        v, a, _ = _run(c, True, rows, k, "euclidean", n_split)
        _same((v, a), _oracle(c, True, rows, k, "euclidean"))
    for q in range(3):
        groups = _groups(c, q, 2)
        if len(groups) >= 3:
            cell_hit = lambda p: ((a[q] >= c["cs"][q, p]) & (a[q] < c["cs"][q, p] + c["sz"][q, p])).any()
            assert any(cell_hit(p) for p in groups[0]) and any(cell_hit(p) for g in groups[2:] for p in g)
            assert not any(cell_hit(p) for p in groups[1])


# ---- 5. rows out of range -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_rows_outside_the_filter_give_pads_and_read_nothing(residual, monkeypatch):
    """filter_of_query = -1 and = n_filters: k pads for that query, the others untouched.  The filter buffer holds
    exactly n_filters * stride words between two guards; the outputs come pre-filled with 0x00, then 0xFF: nothing
    outside them is written, and both fills give the same result -- every output cell is written"""
    c = cases.case(24, 2, 3, 4, "euclidean", residual)
    n_filters, stride = c["bits"].shape
    arena = guarded_alloc.Arena(torch, 0xFF)
    bits = arena.allocate((n_filters, stride), torch.int32, torch.device(DEV), 0xFF, "empty")
    bits.copy_(T(c["bits"].view(np.int32)))
    assert bits.is_contiguous() and bits.numel() == n_filters * stride
    for rows in ([-1, 4, n_filters], [4, n_filters, 0], [-(1 << 31), (1 << 31) - 1, 4]):
        rows = np.array(rows, np.int32)
        for n_split in (1, 5):
            for k in (10, 1024):
                out = guarded_alloc.run_guarded(
                    lambda: _run(c, residual, rows, k, "euclidean", n_split, bits=bits)[:2], monkeypatch=monkeypatch)
                _same(out[0x00], out[0xFF])
                v, a = out[0x00]
                _same((v, a), _oracle(c, residual, rows, k, "euclidean"))
                bad = (rows < 0) | (rows >= n_filters)
                assert np.all(a[bad] == -1) and np.all(np.isneginf(v[bad]))
                clean = _run(c, residual, np.where(bad, 0, rows), k, "euclidean", n_split)
                assert np.array_equal(a[~bad], clean[1][~bad])
                assert np.array_equal(v[~bad].view(np.uint32), clean[0][~bad].view(np.uint32))
    arena.check()


@pytest.mark.parametrize("cid", list(guarded.CASE_SYMBOLS))
def test_guards_hold_and_results_do_not_depend_on_the_fill(cid, monkeypatch):
    """the guarded-buffer cases of the two entry points (tests/ivfpq4_filtered_guarded.py), run as
    tests/test_gpu_guarded_buffers.py runs its own: plainly, then with every output and workspace of the wrapper between
    two canaries and pre-filled with 0x00, then with 0xFF -- the canaries intact (run_guarded raises otherwise), the same
    number of guarded allocations under both fills, and the three results the same bits"""
    from test_gpu_guarded_buffers import same_bits
    fn = guarded.builder(cid.endswith("residual_topk"))()
    want = fn()
    torch.cuda.synchronize()
    got = guarded_alloc.run_guarded(fn, monkeypatch=monkeypatch)
    counts = {fill: len(arena.allocations) for fill, arena in guarded_alloc.run_guarded.arenas.items()}
    assert all(counts.values()) and len(set(counts.values())) == 1, counts
    same_bits(got[0x00], want, f"{cid}: fill 0x00 against the plain call")
    same_bits(got[0xFF], want, f"{cid}: fill 0xFF against the plain call")


# ---- 6. tombstones, free slots, padding -----------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_bits_on_tombstones_free_slots_and_padding_change_nothing(residual):
    c = cases.case(64, 2, 3, 8, "euclidean", residual)
    live = c["is_empty"] == 0
    cap = len(live)
    assert c["allowed"][:, ~live].all()
    strict = dict(c, allowed=c["allowed"] & live)
    strict.pop("gpu", None)
    padded = np.zeros((len(cases.ROWS), ((cap + 31) // 32 + fcases.PAD_WORDS) * 32), bool)
    padded[:, :cap] = strict["allowed"]
    strict["bits"] = forc.pack_bits(padded)            # no bit beyond the live slots, zero padding
    assert not np.array_equal(strict["bits"], c["bits"])
    for rows in c["runs"]:
        for n_split in (None, 1):
            v, a, _ = _run(c, residual, rows, 100, "euclidean", n_split)
            sv, sa, _ = _run(strict, residual, rows, 100, "euclidean", n_split)
            _same((v, a), (sv, sa))
            got = a[a >= 0]
            assert len(got) and live[got].all() and got.max() < cap     # no tombstone, no free slot, nothing beyond


# ---- 7. the summation order ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("n_split", [None, 1])
def test_scan_when_the_summation_order_decides(n_split, residual):
    """ivfpq4_cases.offset_case / ivfpq4_residual_cases.offset_case (partial sums near -2^27, where the order of the
    additions decides the best ten) under a row that allows half the slots"""
    c, k = rcases.offset_case() if residual else pcases.offset_case()
    cap = c["storage"].shape[1]
    c["allowed"] = (np.random.default_rng(99).random((1, cap)) < 0.5) | (c["is_empty"] != 0)
    c["bits"] = fcases.filter_bits(c["allowed"])
    v, a, _ = _run(c, residual, None, k, "inner", n_split)
    _same((v, a), _oracle(c, residual, None, k, "inner"))
    assert (a >= 0).all(1).any()


# ---- 8. NaN ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_a_nan_query_leaves_the_other_lines_alone(residual):
    c = dict(cases.case(64, 2, 3, 8, "euclidean", residual))
    c.pop("gpu", None)
    rows = c["runs"][4]                                 # (rows 4, 0, 1: the half row, everything, nothing)
    clean_v, clean_a, _ = _run(c, residual, rows, 10, "euclidean", 1)
    assert (clean_a[0] >= 0).any()
    for n_split in (1, 3):
        dirty = dict(c, query=c["query"].copy())
        dirty.pop("gpu", None)
        dirty["query"][5, 0] = np.nan
        v, a, _ = _run(dirty, residual, rows, 10, "euclidean", n_split)
        _same((v, a), _oracle(dirty, residual, rows, 10, "euclidean"))
        assert np.array_equal(a[1:], clean_a[1:]) and np.array_equal(v[1:].view(np.uint32), clean_v[1:].view(np.uint32))
        assert np.all(a[0] == -1) and np.all(np.isneginf(v[0]))           # a NaN value never enters


def test_library_declines_what_it_does_not_support():
    from torchpq_amd import _lib
    from torchpq_amd._lib import TorchPQAmdError, check, load, ptr, stream_ptr
    c = cases.case(8, 2, 3, 8, "inner", True)
    g = _gpu(c)
    v, a = torch.empty(3, 5, device=DEV), torch.empty(3, 5, device=DEV, dtype=torch.long)
    n_filters, stride = c["bits"].shape

    def scan(m=8, k=5, n_split=1, n_filters=n_filters, stride=stride):
        return load().tpq_ivfpq4_scan_filtered_residual_topk(
            ptr(g["storage"]), ptr(g["query"]), ptr(g["codebook"]), ptr(g["centroids"]), ptr(g["cells"]),
            len(rcases.CELL_SIZES), ptr(g["is_empty"]), ptr(g["cs"]), ptr(g["sz"]), ptr(g["npl"]), ptr(g["bits"]), None,
            n_filters, stride, ptr(v), ptr(a), g["storage"].shape[1], m, 2, 3, 8, k, 1, n_split, None, 0,
            stream_ptr(DEV))
    for m, k in ((12, 5), (4, 5), (264, 5), (8, 0), (8, 1025)):
        assert scan(m, k) == _lib.ERR_UNSUPPORTED, (m, k)
    assert scan(n_filters=0) == -1 and scan(stride=stride - fcases.PAD_WORDS - 1) == -1
    with pytest.raises(TorchPQAmdError, match="workspace"):                    # the library allocates nothing
        check(scan(n_split=4), "tpq_ivfpq4_scan_filtered_residual_topk")
    assert scan() == 0
    torch.cuda.synchronize()
    _same((N(v), N(a)), _oracle(c, True, None, 5, "inner"))


# ---- 9. the index ----------------------------------------------------------------------------------------------------
D, N_CELLS, N_BASE, NQ = 32, 16, 2000, 24


def _build(distance, residual, m, seed=0):
    """train, add in two batches with explicit ids (tiny initial cells: add forces growth), remove some ids"""
    from torchpq_amd.index import IVFPQ4Index
    base, queries = _clustered(seed, D, N_BASE, NQ)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFPQ4Index(D, n_subvectors=m, n_cells=N_CELLS, initial_size=16, distance=distance, device=DEV,
                      pq_use_residual=residual)
    idx.train(T(base))
    ids = torch.arange(N_BASE, device=DEV) * 2 + 5
    idx.add(T(base[:, :N_BASE // 2]), ids=ids[:N_BASE // 2])
    idx.add(T(base[:, N_BASE // 2:]), ids=ids[N_BASE // 2:])
    removed = np.arange(7, N_BASE, 11)
    idx.remove(ids=ids[T(removed)])
    idx.n_probe = 4
    return idx, base, queries, N(ids), removed


def _expected(idx, queries, id_sets, rows, k):
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    _, cells, npl = idx.probe(T(x))
    centroids = np.ascontiguousarray(N(idx.vq_codec.codebook).T) if idx.pq_use_residual else None
    return forc.search_filtered(x, N(idx.pq_codec.codebook), N(idx._storage), N(idx._is_empty), N(idx._cell_start),
                                N(idx._cell_size), N(idx._address2id), N(cells), N(npl), id_sets, rows, k,
                                idx.distance, centroids=centroids)


def _check(idx, queries, flt, id_sets, rows, k):
    v, i = idx.search_filtered(T(queries), k, flt, None if rows is None else T(rows))
    ev, ei, _ = _expected(idx, queries, id_sets, rows, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and v.shape == i.shape == (queries.shape[1], k)
    assert np.array_equal(N(i), ei)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    return N(v), N(i)


@pytest.mark.parametrize("distance,residual,m", [("euclidean", False, 8), ("cosine", False, 16),
                                                 ("euclidean", True, 16), ("cosine", True, 8)])
def test_index_search_filtered(distance, residual, m):
    idx, base, queries, ids, removed = _build(distance, residual, m, seed=2)
    rng = np.random.default_rng(5)
    # one shared set: a fifth of the ids, removed ones and ids the index never held among them
    fifth = np.concatenate([rng.choice(ids, len(ids) // 5, replace=False), [-3, 4, 10 ** 9]]).astype(np.int64)
    flt = idx.id_filter(T(fifth))
    v, i = _check(idx, queries, flt, [fifth], None, 10)
    found = i[i >= 0]
    assert len(found) and np.isin(found, fifth).all() and not np.isin(found, ids[removed]).any()
    assert not np.array_equal(N(idx.search(T(queries), k=10)[1]), i)       # the filter does change the answer
    # a subset-consistent cut of a full-depth search: the allowed results of search(k = 1024), in its order
    fv, fi = idx.search(T(queries), k=1024)
    fv, fi = N(fv), N(fi)
    assert ((fi >= 0).sum(1) < 1024).all()                                 # full depth: every candidate is in it
    for q in range(NQ):
        keep = (fi[q] >= 0) & np.isin(fi[q], fifth)
        n = min(10, int(keep.sum()))
        assert np.array_equal(i[q][:n], fi[q][keep][:n]) and np.all(i[q][n:] == -1)
        assert np.array_equal(v[q][:n].view(np.uint32), fv[q][keep][:n].view(np.uint32))
    # k larger than the allowed live set pads
    v, i = _check(idx, queries, flt, [fifth], None, 1024)
    assert ((i >= 0).sum(1) < 1024).all() and np.all(np.isneginf(v[i < 0]))
    # filter_of_query chooses among three id sets: everything, one id, a half
    half = ids[rng.random(len(ids)) < 0.5]
    sets = [ids, ids[1234:1235], half]
    multi = idx.id_filter([T(s) for s in sets])
    rows = (np.arange(NQ) % 3).astype(np.int32)
    v, i = _check(idx, queries, multi, sets, rows, 20)
    assert np.array_equal(i[rows == 0], N(idx.search(T(queries), k=20)[1])[rows == 0])    # every id allowed: search
    assert np.all(i[rows == 1][:, 1:] == -1) and set(i[rows == 1][:, 0]) <= {-1, int(ids[1234])}
    v64, i64 = idx.search_filtered(T(queries), 20, multi, T(rows.astype(np.int64)))       # any int tensor chooses
    assert np.array_equal(N(i64), i)
    # a filter made before an add that grows the container gives what one made after gives
    cap_before = idx.capacity
    extra = (base[:, :1500] + 0.01).astype(np.float32)
    new_ids = torch.arange(1500, device=DEV) + 100000
    early = [np.concatenate([half, N(new_ids[::3])]), ids[::7]]
    before = idx.id_filter([T(s) for s in early])
    before.bits()                                                          # built for the old addresses
    idx.add(T(extra), ids=new_ids)
    assert idx.capacity > cap_before
    rows2 = (np.arange(NQ) % 2).astype(np.int32)
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
    cv, ci, ca = idx.search_cells_filtered(x, cells, before, T(rows2), base_sims=sims, n_probe_list=npl, k=50,
                                           return_address=True)
    assert np.array_equal(N(ci), after_remove[1]) and torch.equal(idx.get_id_by_address(ca)[ca >= 0], ci[ca >= 0])
    none = idx.search_filtered(T(queries[:, :0]), 5, before)
    assert none[0].shape == none[1].shape == (0, 5)
    foreign = _build(distance, residual, m, seed=3)[0].id_filter(T(ids[:10]))
    with pytest.raises(AssertionError, match="another index"):
        idx.search_filtered(T(queries), 5, foreign)
