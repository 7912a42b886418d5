"""GPU: IVFPQ4Index range search (tpq_ivfpq4_range_count / _fill and their residual forms, csrc/scan_pq4_range.hip)
against tests/ivfpq4_range_oracle.py -- values compared as uint32, addresses and lims equal -- on the inputs of
tests/ivfpq4_range_cases.py (whose conditions tests/test_ivfpq4_range_cpu.py asserts), against the 4-bit top-k scans
where the two must agree, and the index end to end."""
import numpy as np
import pytest
import torch

import guarded_alloc
import ivfpq4_filtered_cases as fcases
import ivfpq4_range_cases as cases
import ivfpq4_range_guarded as guarded
import ivfpq4_range_oracle as rgo
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _gpu(c):
    """the case's arrays on the GPU, uploaded once"""
    if "gpu" not in c:
        g = {k: T(v) for k, v in c.items() if isinstance(v, np.ndarray) and k not in ("allowed", "bits")}
        g["bits"] = T(c["bits"].view(np.int32))
        c["gpu"] = g
    return c["gpu"]


def _run(c, residual, threshold, distance, run=None, n_split=None, op=None, with_empty=True, rows="run", bits=None):
    """the wrapper on a case: `run` indexes c["runs"] (None: no filter); `rows` overrides the run's filter_of_query"""
    from torchpq_amd.kernels import IVFPQ4RangeHip
    g = _gpu(c)
    op = op or IVFPQ4RangeHip(m=c["codebook"].shape[0])
    kw = dict(is_empty=g["is_empty"] if with_empty else None, distance=distance)
    if run is not None or bits is not None or not isinstance(rows, str):
        rows = c["runs"][run] if isinstance(rows, str) else rows
        kw.update(filter_bits=g["bits"] if bits is None else bits,
                  filter_of_query=None if rows is None else T(np.asarray(rows, np.int32)))
    thr = T(np.asarray(threshold, np.float32)) if isinstance(threshold, np.ndarray) else threshold
    if residual:
        lims, v, a = op.residual(g["storage"], g["query"], g["codebook"], g["centroids"], g["cells"], g["cs"], g["sz"],
                                 g["npl"], thr, **kw)
    else:
        lims, v, a = op(g["storage"], g["query"], g["codebook"], g["cs"], g["sz"], g["npl"], thr, n_split=n_split, **kw)
    nq = c["query"].shape[1]
    assert lims.dtype == torch.int64 and v.dtype == torch.float32 and a.dtype == torch.int64
    assert lims.shape == (nq + 1,) and v.shape == a.shape == (int(lims[-1]),) and int(lims[0]) == 0
    return N(lims), N(v), N(a), op


def _same(got, want):
    assert np.array_equal(got[0], want[0])
    assert np.array_equal(got[2], want[2])
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


# ---- 1. the wrapper against the oracle -----------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", cases.KERNEL_CASES)
def test_range_against_the_oracle(m, ds, nq, n_probe, distance, residual):
    """every threshold set and (plain codes) every n_split give the oracle's lims, addresses and value bits, hence the
    same bits and order as every other split; with and without is_empty"""
    from torchpq_amd.kernels import IVFPQ4RangeHip
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    op = IVFPQ4RangeHip(m=m)
    splits = (None,) if residual or nq > 3 else cases.SPLITS
    for with_empty in (True, False):
        cand = cases.candidates(c, residual, distance, with_empty=with_empty)
        thr = cases.thresholds(cand)
        n_hits = 0
        for name, t in thr.items():
            want = rgo.hits(cand, t)
            n_hits += len(want[1])
            for n_split in splits:
                got = _run(c, residual, t, distance, n_split=n_split, op=op, with_empty=with_empty)
                _same(got, want)
                if not residual:
                    if n_split is None:   # a small batch is split over several workgroups, a large one left whole
                        assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
                    else:
                        assert op.last_n_split == n_split
            if not with_empty and nq > 3:
                break                      # (the large batch without tombstones: one threshold set)
        assert n_hits > 0
    # a Python float is one threshold for every query
    cand = cases.candidates(c, residual, distance)
    t = float(cases.thresholds(cand)["median"][0])
    _same(_run(c, residual, t, distance, op=op), rgo.hits(cand, t))


# ---- 2. the filter -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", cases.KERNEL_CASES)
def test_filtered_range_against_the_oracle(m, ds, nq, n_probe, distance, residual):
    """every run of filter rows -- single, sparse and half rows, mixed per query in one call; the last run passes no
    filter_of_query: row 0 -- under the median, the boundary and the mixed thresholds"""
    from torchpq_amd.kernels import IVFPQ4RangeHip
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    op = IVFPQ4RangeHip(m=m)
    live = c["is_empty"] == 0
    n_hits = 0
    for run, rows in enumerate(c["runs"]):
        cand = cases.candidates(c, residual, distance, run=run)
        thr = cases.thresholds(cand)
        for name in ("median", "boundary", "above", "mixed0") if nq > 1 else ("median", "boundary", "minus_inf"):
            want = rgo.hits(cand, thr[name])
            for n_split in ((None,) if residual or nq > 3 else (None, 1, 7)):
                got = _run(c, residual, thr[name], distance, run=run, n_split=n_split, op=op)
                _same(got, want)
            n_hits += len(want[2])
            assert live[want[2]].all()                  # bits on tombstones and free slots never produce a hit
    assert n_hits > 0


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_all_ones_row_is_the_unfiltered_call_and_rows_without_bits_give_nothing(distance, residual):
    c = cases.case(24, 2, 3, 4, "euclidean", residual)
    cand = cases.candidates(c, residual, distance)
    thr = cases.thresholds(cand)
    n_filters = len(cases.ROWS)
    for n_split in (1, 3):
        for name in ("median", "mixed0"):
            plain = _run(c, residual, thr[name], distance, n_split=n_split)
            assert len(plain[1]) > 0
            for rows in (None, np.zeros(3, np.int32)):
                _same(_run(c, residual, thr[name], distance, rows=rows, n_split=n_split), plain)
        everything = np.full(3, -np.inf, np.float32)
        # the zeros row, and rows outside [0, n_filters): no hit
        for rows in ([1, 1, 1], [-1, n_filters, 1], [-(1 << 31), (1 << 31) - 1, n_filters + 5]):
            lims, v, a, _ = _run(c, residual, everything, distance, rows=np.array(rows, np.int32), n_split=n_split)
            assert np.array_equal(lims, np.zeros(4, np.int64)) and len(v) == len(a) == 0
        # ... next to a query with a row: only that query's segment is filled, with what it has on its own
        rows = np.array([0, -1, n_filters], np.int32)
        got = _run(c, residual, everything, distance, rows=rows, n_split=n_split)
        want = rgo.hits([(s, v) if q == 0 else (s[:0], v[:0]) for q, (s, v) in enumerate(cand)], everything)
        _same(got, want)
        assert got[0][1] == got[0][2] == got[0][3] > 0


def test_rows_outside_the_filter_read_nothing(monkeypatch):
    """the filter buffer holds exactly n_filters * stride words between two guards"""
    c = cases.case(24, 2, 3, 4, "euclidean", True)
    n_filters, stride = c["bits"].shape
    arena = guarded_alloc.Arena(torch, 0xFF)
    bits = arena.allocate((n_filters, stride), torch.int32, torch.device(DEV), 0xFF, "empty")
    bits.copy_(T(c["bits"].view(np.int32)))
    rows = np.array([4, -1, n_filters], np.int32)
    everything = np.full(3, -np.inf, np.float32)
    for residual in (False, True):
        cand = cases.candidates(c, residual, "euclidean", run=None)
        allowed = (c["allowed"][4] & (c["is_empty"] == 0))
        out = guarded_alloc.run_guarded(lambda: _run(c, residual, everything, "euclidean", rows=rows, bits=bits)[:3],
                                        monkeypatch=monkeypatch)
        _same(out[0x00], out[0xFF])
        s, v = cand[0]
        want = rgo.hits([(s[allowed[s]], v[allowed[s]]), (s[:0], v[:0]), (s[:0], v[:0])], everything)
        _same(out[0x00], want)
        assert len(want[1]) > 0
    arena.check()


# ---- 3. residual specifics -----------------------------------------------------------------------------------------
def test_every_tile_is_valued_in_its_own_probes_table():
    """every slot holds the same code, so a value depends on the probe's centroid alone: all hits of one probe carry
    one value, the probes' values differ, and they are the oracle's"""
    c = fcases.mixed_table_case()
    cap = c["storage"].shape[1]
    everything = np.full(3, -np.inf, np.float32)
    for run, kw in ((None, {}), (0, dict(rows=np.zeros(3, np.int32))), (1, dict(rows=np.ones(3, np.int32)))):
        flt = {} if run is None else dict(allowed=c["allowed"], rows=kw["rows"])
        cand = rgo.candidates(c["storage"], c["query"], c["codebook"], c["is_empty"], c["cs"], c["sz"], c["npl"],
                              "euclidean", centroids=c["centroids"], cells=c["cells"], probes=True, **flt)
        got = _run(c, True, everything, "euclidean", **kw)
        _same(got, rgo.hits([t[:2] for t in cand], everything))
        lims, v, a, _ = got
        for q, (s, _, p) in enumerate(cand):
            vq = v[lims[q]:lims[q + 1]]
            assert np.array_equal(a[lims[q]:lims[q + 1]], s)
            for rank in np.unique(p):
                assert len(np.unique(vq[p == rank])) == 1
            if run is None and len(np.unique(p)) >= 3:
                assert len(np.unique(vq)) >= 3
    assert len(v) > 0 and a.max() < cap


def test_segment_counts_a_skipped_duplicate_probe_has_eight_zero_counts():
    """the count pass itself, against the segment model of tests/ivfpq4_range_cases.segment_counts: the (query, probe)
    segments of residual codes and the (query, part) segments of plain codes at n_split = 1 and 5"""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    c = cases.case(24, 2, 3, 4, "euclidean", True)
    g = _gpu(c)
    nq, n_probe = c["cs"].shape
    n_slots = c["storage"].shape[1]
    for residual in (True, False):
        cand_p = cases.candidates(c, residual, "euclidean", probes=True)
        thr = cases.thresholds([t[:2] for t in cand_p])["median"]
        t_gpu = T(thr)
        for n_split in ((1,) if residual else (1, 5)):
            if residual:
                n_seg = lib.tpq_ivfpq4_range_residual_segments(nq, n_probe)
                counts = torch.full((n_seg,), -5, device=DEV, dtype=torch.int32)
                check(lib.tpq_ivfpq4_range_residual_count(
                    ptr(g["storage"]), ptr(g["query"]), ptr(g["codebook"]), ptr(g["centroids"]), ptr(g["cells"]),
                    c["centroids"].shape[0], ptr(g["is_empty"]), ptr(g["cs"]), ptr(g["sz"]), ptr(g["npl"]), None, None,
                    0, 0, ptr(t_gpu), ptr(counts), n_slots, 24, 2, nq, n_probe, 0, stream_ptr(DEV)), "count")
            else:
                n_seg = lib.tpq_ivfpq4_range_segments(nq, n_split)
                counts = torch.full((n_seg,), -5, device=DEV, dtype=torch.int32)
                check(lib.tpq_ivfpq4_range_count(
                    ptr(g["storage"]), ptr(g["query"]), ptr(g["codebook"]), ptr(g["is_empty"]), ptr(g["cs"]),
                    ptr(g["sz"]), ptr(g["npl"]), None, None, 0, 0, ptr(t_gpu), ptr(counts), n_slots, 24, 2, nq,
                    n_probe, 0, n_split, stream_ptr(DEV)), "count")
            torch.cuda.synchronize()
            want = cases.segment_counts(c, cand_p, thr, residual, n_split)
            assert np.array_equal(N(counts).reshape(want.shape), want)
            assert want.sum() > 0
            if residual:
                assert c["cs"][1, 1] == c["cs"][1, 0] and np.all(N(counts).reshape(want.shape)[1, 1] == 0)
                assert not (N(counts) < 0).any()                    # every segment is written, the unscanned ones too


def test_a_slot_of_two_overlapping_cells_appears_once_per_probe():
    c = cases.overlap_case()
    everything = np.full(1, -np.inf, np.float32)
    cand = rgo.candidates(c["storage"], c["query"], c["codebook"], c["is_empty"], c["cs"], c["sz"], c["npl"],
                          "euclidean", centroids=c["centroids"], cells=c["cells"], probes=True)
    got = _run(c, True, everything, "euclidean")
    _same(got, rgo.hits([t[:2] for t in cand], everything))
    s, v, p = cand[0]
    twice = np.intersect1d(s[p == 0], s[p == 1])
    assert len(twice) > 20
    for slot in twice:
        at = np.flatnonzero(got[2] == slot)
        assert len(at) == 2 and got[1][at[0]] != got[1][at[1]]          # each time in its own probe's table


# ---- 4. the top-k scans --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", [k for k in cases.KERNEL_CASES if k[2] <= 3])
def test_hits_at_minus_inf_sorted_are_the_topk_scans(m, ds, nq, n_probe, distance, residual):
    from torchpq_amd.kernels import IVFPQ4FilteredTopkHip, IVFPQ4ResidualTopkHip, IVFPQ4TopkHip
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    g = _gpu(c)
    everything = np.full(nq, -np.inf, np.float32)
    k = 1024
    rows = c["runs"][0]
    for filtered in (False, True):
        lims, v, a, _ = _run(c, residual, everything, distance, **(dict(rows=rows) if filtered else {}))
        sv, sa = rgo.sort_segments(lims, v, a)
        tables = (g["centroids"], g["cells"]) if residual else ()
        if filtered:
            op = IVFPQ4FilteredTopkHip(m=m)
            tv, ta = (op.residual if residual else op)(
                g["storage"], g["query"], g["codebook"], *tables, g["cs"], g["sz"], g["npl"], k, g["bits"],
                filter_of_query=T(rows), is_empty=g["is_empty"], distance=distance)
        else:
            tv, ta = (IVFPQ4ResidualTopkHip if residual else IVFPQ4TopkHip)(m=m)(
                g["storage"], g["query"], g["codebook"], *tables, g["cs"], g["sz"], g["npl"], k,
                is_empty=g["is_empty"], distance=distance)
        tv, ta = N(tv), N(ta)
        seen = 0
        for q in range(nq):
            n = int(min(lims[q + 1] - lims[q], k))
            assert np.array_equal(sa[lims[q]:lims[q] + n], ta[q, :n]) and np.all(ta[q, n:] == -1)
            assert np.array_equal(sv[lims[q]:lims[q] + n].view(np.uint32), tv[q, :n].view(np.uint32))
            seen += n
        assert seen > 0


# ---- 5. NaN --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
def test_a_nan_query_leaves_the_other_queries_segments_alone(residual):
    c = dict(cases.case(64, 2, 3, 8, "euclidean", residual))
    for key in [k for k in c if k == "gpu" or isinstance(k, tuple)]:
        c.pop(key)
    cand = cases.candidates(c, residual, "euclidean")
    thr = cases.thresholds(cand)["median"]
    clean = _run(c, residual, thr, "euclidean", n_split=1)
    assert clean[0][1] > 0
    dirty = dict(c, query=c["query"].copy())
    for key in [k for k in dirty if k == "gpu" or isinstance(k, tuple)]:
        dirty.pop(key)
    dirty["query"][5, 0] = np.nan
    for n_split in (1, 3):
        got = _run(dirty, residual, thr, "euclidean", n_split=n_split)
        _same(got, rgo.hits(cases.candidates(dirty, residual, "euclidean"), thr))
        assert got[0][1] == 0                                            # a NaN value is never a hit
        lo, clo = got[0][1], clean[0][1]
        assert np.array_equal(got[2][lo:], clean[2][clo:])
        assert np.array_equal(got[1][lo:].view(np.uint32), clean[1][clo:].view(np.uint32))


# ---- 6. the fill pass stays inside its segments --------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "residual", "plain_filtered", "residual_filtered"])
def test_fill_never_writes_beyond_a_segment_when_the_inputs_changed(form):
    """counts from a selective threshold, then a fill pass with -inf (every candidate a hit): each wave stores its
    first wave_count hits and nothing at or beyond the next segment's offset.  The outputs are as long as an unguarded
    fill would need, and hold a canary."""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    residual, filtered = form.startswith("residual"), form.endswith("filtered")
    c = cases.case(24, 2, 3, 4, "euclidean", residual)
    g = _gpu(c)
    nq, n_probe = c["cs"].shape
    n_split, n_slots = 3, c["storage"].shape[1]
    run = len(c["runs"]) - 2 if filtered else None
    rows = T(c["runs"][run]) if filtered else None
    flt = [ptr(g["bits"]), ptr(rows), c["bits"].shape[0], c["bits"].shape[1]] if filtered else [None, None, 0, 0]
    lists = [ptr(g["is_empty"]), ptr(g["cs"]), ptr(g["sz"]), ptr(g["npl"])] + flt
    if residual:
        n_seg, per_query = lib.tpq_ivfpq4_range_residual_segments(nq, n_probe), n_probe * 8
        inputs = [ptr(g["storage"]), ptr(g["query"]), ptr(g["codebook"]), ptr(g["centroids"]), ptr(g["cells"]),
                  c["centroids"].shape[0]] + lists
        shape = (n_slots, 24, 2, nq, n_probe, 0, stream_ptr(DEV))
        count, fill = lib.tpq_ivfpq4_range_residual_count, lib.tpq_ivfpq4_range_residual_fill
    else:
        n_seg, per_query = lib.tpq_ivfpq4_range_segments(nq, n_split), n_split * 8
        inputs = [ptr(g["storage"]), ptr(g["query"]), ptr(g["codebook"])] + lists
        shape = (n_slots, 24, 2, nq, n_probe, 0, n_split, stream_ptr(DEV))
        count, fill = lib.tpq_ivfpq4_range_count, lib.tpq_ivfpq4_range_fill
    assert n_seg == nq * per_query
    cand = cases.candidates(c, residual, "euclidean", run=run)
    counts = torch.empty(n_seg, device=DEV, dtype=torch.int32)
    t_count, t_fill = T(cases.thresholds(cand)["median"]), torch.full((nq,), -np.inf, device=DEV)
    check(count(*inputs, ptr(t_count), ptr(counts), *shape), "count")
    offsets = torch.zeros(n_seg + 1, device=DEV, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0)
    total, n_all = int(offsets[-1]), sum(len(s) for s, _ in cand)
    assert 0 < total < n_all
    assert np.array_equal(N(offsets)[::per_query], rgo.hits(cand, N(t_count))[0])
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


@pytest.mark.parametrize("cid", list(guarded.CASE_SYMBOLS))
def test_guards_hold_and_results_do_not_depend_on_the_fill(cid, monkeypatch):
    """the guarded-buffer cases of the four entry points (tests/ivfpq4_range_guarded.py), run as
    tests/test_gpu_guarded_buffers.py runs its own: plainly, then with every output and workspace of the wrapper between
    two canaries and pre-filled with 0x00, then with 0xFF -- the canaries intact (run_guarded raises otherwise), the same
    number of guarded allocations under both fills, and the three results the same bits"""
    from test_gpu_guarded_buffers import same_bits
    fn = guarded.builder(cid.endswith("residual"))()
    want = fn()
    torch.cuda.synchronize()
    got = guarded_alloc.run_guarded(fn, monkeypatch=monkeypatch)
    counts = {fill: len(arena.allocations) for fill, arena in guarded_alloc.run_guarded.arenas.items()}
    assert all(counts.values()) and len(set(counts.values())) == 1, counts
    same_bits(got[0x00], want, f"{cid}: fill 0x00 against the plain call")
    same_bits(got[0xFF], want, f"{cid}: fill 0xFF against the plain call")


def test_library_declines_what_it_does_not_support():
    from torchpq_amd import _lib
    from torchpq_amd._lib import load, ptr, stream_ptr
    c = cases.case(8, 2, 3, 8, "inner", True)
    g = _gpu(c)
    n_filters, stride = c["bits"].shape
    counts = torch.empty(3 * 8 * 8, device=DEV, dtype=torch.int32)
    thr = torch.full((3,), -np.inf, device=DEV)

    def count(m=8, n_filters=n_filters, stride=stride, n_cells=8, metric=1):
        return load().tpq_ivfpq4_range_residual_count(
            ptr(g["storage"]), ptr(g["query"]), ptr(g["codebook"]), ptr(g["centroids"]), ptr(g["cells"]), n_cells,
            ptr(g["is_empty"]), ptr(g["cs"]), ptr(g["sz"]), ptr(g["npl"]), ptr(g["bits"]), None, n_filters, stride,
            ptr(thr), ptr(counts), g["storage"].shape[1], m, 2, 3, 8, metric, stream_ptr(DEV))
    for m in (12, 4, 264):
        assert count(m) == _lib.ERR_UNSUPPORTED, m
    assert count(n_filters=0) == -1 and count(stride=stride - fcases.fcases.PAD_WORDS - 1) == -1
    assert count(n_cells=0) == -1 and count(metric=7) == -1
    assert count() == 0
    torch.cuda.synchronize()
    cand = cases.candidates(c, True, "inner", run=len(c["runs"]) - 1)
    assert N(counts).sum() == sum(len(s) for s, _ in cand) > 0


# ---- 7. the index --------------------------------------------------------------------------------------------------
D, N_CELLS, N_BASE, NQ = 32, 16, 2000, 5


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


def _expected(idx, queries, threshold, id_sets=None, rows=None):
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    _, cells, npl = idx.probe(T(x))
    centroids = np.ascontiguousarray(N(idx.vq_codec.codebook).T) if idx.pq_use_residual else None
    return rgo.range_search(x, N(idx.pq_codec.codebook), N(idx._storage), N(idx._is_empty), N(idx._cell_start),
                            N(idx._cell_size), N(idx._address2id), N(cells), N(npl), threshold, idx.distance,
                            centroids=centroids, id_sets=id_sets, rows=rows)


def _check(idx, queries, threshold, flt=None, id_sets=None, rows=None, sort=False):
    thr = T(threshold) if isinstance(threshold, np.ndarray) else threshold
    if flt is None:
        got = idx.range_search(T(queries), thr, return_address=True, sort=sort)
    else:
        got = idx.range_search_filtered(T(queries), thr, flt, None if rows is None else T(rows), return_address=True,
                                        sort=sort)
    lims, v, i, a = (N(t) for t in got)
    el, ev, ei, ea = _expected(idx, queries, threshold, id_sets, rows)
    if sort:
        ev, ea, ei = rgo.sort_segments(el, ev, ea, ei)
    assert got[0].dtype == got[2].dtype == got[3].dtype == torch.int64 and got[1].dtype == torch.float32
    assert np.array_equal(lims, el) and np.array_equal(a, ea) and np.array_equal(i, ei)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    return lims, v, i, a


@pytest.mark.parametrize("distance,residual,m", [("euclidean", False, 8), ("cosine", False, 16),
                                                 ("euclidean", True, 16), ("cosine", True, 8)])
def test_index_range_search(distance, residual, m):
    idx, base, queries, ids, removed = _build(distance, residual, m, seed=2)
    assert idx.capacity > 16 * N_CELLS                                   # the adds grew the container
    # the thresholds: every query's 20th value of search
    tv, ti = idx.search(T(queries), k=20)
    thr = N(tv[:, -1]).copy()
    assert np.isfinite(thr).all()
    lims, v, i, a = _check(idx, queries, thr)
    assert (np.diff(lims) >= 20).all() and not np.isin(i, ids[removed]).any()
    lims2, v2, i2 = (N(t) for t in idx.range_search(T(queries), T(thr)))  # without the addresses
    assert np.array_equal(lims2, lims) and np.array_equal(i2, i)
    # a scalar threshold, sorted
    scalar = float(np.median(thr))
    lims, v, i, a = _check(idx, queries, scalar, sort=True)
    assert len(v) > 0
    for q in range(NQ):
        assert np.all(np.diff(v[lims[q]:lims[q + 1]]) <= 0)
    # max_query_batch = 2 with 5 queries: the lims of the later batches are offset
    whole = _check(idx, queries, thr, sort=True)
    idx.max_query_batch = 2
    batched = _check(idx, queries, thr, sort=True)
    unsorted_batched = _check(idx, queries, thr)
    idx.max_query_batch = 32768
    for x, y in zip(batched, whole):
        assert np.array_equal(x, y)
    assert len(unsorted_batched[1]) == len(whole[1])
    # search(k) is the first k of range_search(-inf, sort=True)
    lims, v, i, a = _check(idx, queries, -np.inf, sort=True)
    for q in range(NQ):
        n = int(min(20, lims[q + 1] - lims[q]))
        assert n == 20
        assert np.array_equal(i[lims[q]:lims[q] + n], N(ti)[q, :n])
        assert np.array_equal(v[lims[q]:lims[q] + n].view(np.uint32), N(tv)[q, :n].view(np.uint32))
    # filtered: a shared set, then a row per query (everything, one id, a half, and a row outside the filter)
    rng = np.random.default_rng(5)
    fifth = np.concatenate([rng.choice(ids, len(ids) // 5, replace=False), [-3, 4, 10 ** 9]]).astype(np.int64)
    flt = idx.id_filter(T(fifth))
    lims, v, i, a = _check(idx, queries, thr * 4 if distance == "euclidean" else thr - 0.5, flt, [fifth])
    assert len(i) and np.isin(i, fifth).all() and not np.isin(i, ids[removed]).any()
    half = ids[rng.random(len(ids)) < 0.5]
    sets = [ids, ids[1234:1235], half]
    multi = idx.id_filter([T(s) for s in sets])
    rows = np.array([0, 1, 2, 3, 2], np.int32)
    lims, v, i, a = _check(idx, queries, -np.inf, multi, sets, rows, sort=True)
    plain = _check(idx, queries, -np.inf, sort=True)
    assert np.array_equal(i[lims[0]:lims[1]], plain[2][plain[0][0]:plain[0][1]])     # every id allowed: range_search
    assert lims[2] - lims[1] <= 1 and lims[4] == lims[3] and lims[5] > lims[4]
    got64 = idx.range_search_filtered(T(queries), -np.inf, multi, T(rows.astype(np.int64)), sort=True)
    assert np.array_equal(N(got64[2]), i)                                             # any int tensor chooses
    idx.max_query_batch = 2                                                           # the rows are cut alongside
    batched = _check(idx, queries, -np.inf, multi, sets, rows, sort=True)
    idx.max_query_batch = 32768
    assert np.array_equal(batched[0], lims) and np.array_equal(batched[2], i)
    # a filter made before an add that grows the container gives what one made after gives, and follows a remove
    cap_before = idx.capacity
    extra = (base[:, :1500] + 0.01).astype(np.float32)
    new_ids = torch.arange(1500, device=DEV) + 100000
    early = [np.concatenate([half, N(new_ids[::3])]), ids[::7]]
    before = idx.id_filter([T(s) for s in early])
    before.bits()                                                                     # built for the old addresses
    idx.add(T(extra), ids=new_ids)
    assert idx.capacity > cap_before
    rows2 = (np.arange(NQ) % 2).astype(np.int32)
    got_before = _check(idx, queries, thr, before, early, rows2)
    got_after = _check(idx, queries, thr, idx.id_filter([T(s) for s in early]), early, rows2)
    assert np.array_equal(got_before[2], got_after[2]) and np.isin(got_before[2], N(new_ids)).any()
    gone = np.unique(got_before[2][:5])
    idx.remove(ids=T(gone))
    after_remove = _check(idx, queries, thr, before, early, rows2)
    assert not np.isin(after_remove[2], gone).any()
    _check(idx, queries, thr)                                                         # ... and the unfiltered search too
    # range_search_cells(_filtered) on the caller's cells; the empty batch
    x = idx._prepare(T(queries))
    sims, cells, npl = idx.probe(x)
    cl, cv, ci = idx.range_search_cells_filtered(x, cells, T(thr), before, T(rows2), base_sims=sims, n_probe_list=npl)
    assert np.array_equal(N(ci), after_remove[2]) and np.array_equal(N(cl), after_remove[0])
    cl, cv, ci, ca = idx.range_search_cells(x, cells, T(thr), base_sims=sims, n_probe_list=npl, return_address=True)
    assert torch.equal(idx.get_id_by_address(ca), ci) and int(cl[-1]) == len(ci) > 0
    none = idx.range_search(T(queries[:, :0]), 0.0)
    assert N(none[0]).tolist() == [0] and len(none[1]) == len(none[2]) == 0
    none = idx.range_search_filtered(T(queries[:, :0]), 0.0, before, return_address=True)
    assert N(none[0]).tolist() == [0] and len(none) == 4
    foreign = _build(distance, residual, m, seed=3)[0].id_filter(T(ids[:10]))
    with pytest.raises(AssertionError, match="another index"):
        idx.range_search_filtered(T(queries), 0.0, foreign)
