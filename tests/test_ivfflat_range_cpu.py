"""CPU: the surface of IVFFlatIndex range search -- the three C-ABI symbols and their validation, the wrapper and the
index methods -- and the range oracle (tests/ivfflat_range_oracle.py) pinned against float64 brute force where fp32
is exact."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ivfflat_range_oracle as rorc
from conftest import ROOT

RANGE_SYMBOLS = ("tpq_ivfflat_range_segments", "tpq_ivfflat_range_count", "tpq_ivfflat_range_fill")


def test_symbols_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in RANGE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
    assert "value >= threshold[q]" in header and "probe rank ascending, then address ascending" in header
    assert "allocates nothing" in header
    lib = _lib.load()
    assert lib.tpq_version() == 500
    assert lib.tpq_ivfflat_range_segments(7, 3) == 168
    for nq, n_split in ((0, 1), (-1, 1), (5, 0), (5, 1025)):
        assert lib.tpq_ivfflat_range_segments(nq, n_split) == 0
    # validation comes before any HIP call; the table is tpq_ivfflat_scan_topk's (tests/test_ivfflat_cpu.py) without k
    #               vectors query empty start size npl  thr   counts n_slots d  nq np metric split stream
    count = ("tpq_ivfflat_range_count", [None, None, None, None, None, None, None, None, 100, 8, 1, 4, 0, 1, None], 8)
    #              vectors query empty start size npl  thr   offs  vals  addr  n_slots d  nq np metric split stream
    fill = ("tpq_ivfflat_range_fill", [None, None, None, None, None, None, None, None, None, None, 100, 8, 1, 4, 0, 1,
                                       None], 10)
    for name, args, n0 in (count, fill):
        fn = getattr(lib, name)
        assert fn(*args) == -1 and "null pointer" in _lib.last_error()
        # d = 0, metric = 2, n_split = 0, n_split = 1025, max_nprobe = 0
        for pos, bad in ((n0 + 1, 0), (n0 + 4, 2), (n0 + 5, 0), (n0 + 5, 1025), (n0 + 3, 0)):
            a = list(args)
            a[pos] = bad
            assert fn(*a) == -1 and "null pointer" not in _lib.last_error(), (name, pos, bad)
        a = list(args)
        a[n0] = (1 << 31) - 1
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
        a = list(args)
        a[n0 + 2] = 0
        assert fn(*a) == 0  # no queries: nothing to do


def test_wrapper_and_index_methods_exist():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    assert "IVFFlatRangeHip" in kernels.__all__ and callable(kernels.IVFFlatRangeHip)
    sig = inspect.signature(kernels.IVFFlatRangeHip.__call__)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("vectors", inspect.Parameter.empty), ("query", inspect.Parameter.empty),
        ("cell_start", inspect.Parameter.empty), ("cell_size", inspect.Parameter.empty),
        ("n_probe_list", inspect.Parameter.empty), ("threshold", inspect.Parameter.empty), ("is_empty", None),
        ("distance", "euclidean"), ("n_split", None), ("slots_hint", None)]
    assert kernels.IVFFlatRangeHip().last_n_split is None
    sig = inspect.signature(index.IVFFlatIndex.range_search)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("x", inspect.Parameter.empty), ("threshold", inspect.Parameter.empty), ("return_address", False),
        ("sort", False)]
    sig = inspect.signature(index.IVFFlatIndex.range_search_cells)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("x", inspect.Parameter.empty), ("cells", inspect.Parameter.empty), ("threshold", inspect.Parameter.empty),
        ("n_probe_list", None), ("return_address", False), ("_extents", None)]
    doc = index.IVFFlatIndex.range_search.__doc__
    assert "-squared-L2" in doc and "cosine similarity" in doc      # the threshold's value space is stated


def test_wrapper_declines_cpu_tensors_and_a_float64_threshold():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFFlatRangeHip
    vec, q = torch.zeros(4, 100), torch.zeros(4, 2)
    cs, sz, npl = torch.zeros(2, 1, dtype=torch.long), torch.full((2, 1), 10), torch.ones(2, dtype=torch.long)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        IVFFlatRangeHip()(vec, q, cs, sz, npl, -1.0)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        IVFFlatRangeHip()(vec, q, cs, sz, npl, torch.zeros(2))
    with pytest.raises(AssertionError):
        IVFFlatRangeHip()(vec, q, cs, sz, npl, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(AssertionError):
        IVFFlatRangeHip()(vec, q, cs, sz, npl, torch.zeros(3))           # one threshold per query
    with pytest.raises(AssertionError):
        IVFFlatRangeHip()(vec.double(), q, cs, sz, npl, -1.0)


def _integer_data(seed, d, n, nq):
    """SIFT-like: integer components 0 ... 218"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 219, (d, n)).astype(np.float32), rng.integers(0, 219, (d, nq)).astype(np.float32))


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_oracle_equals_float64_brute_force_on_integer_data(distance):
    """d = 32, components 0 ... 218: every partial sum is an integer below 32 * 218^2 < 2^24, so fp32 is exact -- the
    hits must EQUAL the float64 result.  Query 0's threshold lies exactly on the value of thirty equal vectors: the
    compare is inclusive, all thirty are hits."""
    d, n_cells, per_cell, nq = 32, 12, 90, 9
    cap = n_cells * per_cell
    base, query = _integer_data(3, d, cap, nq)
    base[:, 100:130] = base[:, 40:41]        # thirty copies of one vector (cell 1, slots 10 ... 39)
    rng = np.random.default_rng(4)
    sizes = rng.integers(0, per_cell + 1, n_cells).astype(np.int64)
    sizes[1] = per_cell
    start = (np.arange(n_cells) * per_cell).astype(np.int64)
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    tomb = rng.choice(np.setdiff1d(np.arange(cap), np.arange(100, 130)), 60, replace=False)
    is_empty[tomb] = 1                        # tombstones inside the cells
    cells = np.stack([rng.permutation(n_cells)[:5] for _ in range(nq)])
    cells[0] = [3, 1, 0, 5, 7]                # query 0 probes the cell of the copies
    npl = rng.integers(1, 6, nq).astype(np.int64)
    npl[0] = 5
    b64, q64 = base.astype(np.float64), query.astype(np.float64)

    def exact(q, slots):
        diff = q64[:, q:q + 1] - b64[:, slots]
        return -(diff * diff).sum(0) if distance == "euclidean" else (q64[:, q:q + 1] * b64[:, slots]).sum(0)

    # per-query thresholds: the tied value for query 0, a middle candidate's value for the others
    slots_of = []
    for q in range(nq):
        slots = np.concatenate([np.arange(start[c], start[c] + sizes[c]) for c in cells[q, :npl[q]]])
        slots_of.append(slots[is_empty[slots] == 0])
    thr = np.array([np.sort(exact(q, slots_of[q]))[len(slots_of[q]) // 2] for q in range(nq)], np.float32)
    thr[0] = exact(0, np.array([100]))[0]
    lims, v, a = rorc.range_scan(base, query, is_empty, start[cells], sizes[cells], npl, thr, distance)
    assert lims.dtype == np.int64 and v.dtype == np.float32 and a.dtype == np.int64
    assert lims[0] == 0 and lims[-1] == len(v) == len(a) and np.all(np.diff(lims) >= 0)
    for q in range(nq):
        e = exact(q, slots_of[q])
        assert np.abs(e).max() < 2 ** 24
        keep = e >= float(thr[q])
        seg = slice(lims[q], lims[q + 1])
        assert np.array_equal(a[seg], slots_of[q][keep])                 # scan order: probe rank, then address
        assert np.array_equal(v[seg].astype(np.float64), e[keep])
    seg0 = a[lims[0]:lims[1]]
    assert np.isin(np.arange(100, 130), seg0).all()                      # on the threshold: all thirty are hits
    assert np.all(v[lims[0]:lims[1]][np.isin(seg0, np.arange(100, 130))] == thr[0])
    above = np.nextafter(thr[0], np.float32(np.inf))
    _, _, a_up = rorc.range_scan(base, query[:, :1], is_empty, start[cells[:1]], sizes[cells[:1]], npl[:1], above,
                                 distance)
    assert not np.isin(np.arange(100, 130), a_up).any()                  # one ulp above: none of them
    # sorted form: value descending, address ascending
    sv, sa = rorc.sort_segments(lims, v, a)
    for q in range(nq):
        seg = slice(lims[q], lims[q + 1])
        assert np.array_equal(np.lexsort((sa[seg], -sv[seg].astype(np.float64))), np.arange(lims[q + 1] - lims[q]))
        assert sorted(sa[seg]) == sorted(a[seg])


def test_oracle_probe_rules_thresholds_and_nan():
    d, cap = 3, 64
    rng = np.random.default_rng(0)
    base = rng.standard_normal((d, cap)).astype(np.float32)
    query = rng.standard_normal((d, 4)).astype(np.float32)
    start = np.array([[16, 16, 0, 32]] * 4, np.int64)     # the second probe repeats the first: skipped
    size = np.array([[16, 16, 16, -3]] * 4, np.int64)     # a negative size is an empty cell
    is_empty = np.zeros(cap, np.uint8)
    is_empty[[3, 22]] = 1
    npl = np.array([9, 4, 1, 0], np.int64)                # clamped to [0, 4]
    live = [s for s in range(16, 32) if s != 22] + [s for s in range(16) if s != 3]    # probe rank, then address
    lims, v, a = rorc.range_scan(base, query, is_empty, start, size, npl, -np.inf)
    assert list(lims) == [0, 30, 60, 75, 75]
    assert list(a[:30]) == live and list(a[30:60]) == live and list(a[60:75]) == live[:15]
    # +inf and NaN thresholds: nothing; per-query thresholds are per query
    for t in (np.inf, np.nan):
        lims_t, v_t, a_t = rorc.range_scan(base, query, is_empty, start, size, npl, t)
        assert list(lims_t) == [0] * 5 and len(v_t) == len(a_t) == 0
    thr = np.array([-np.inf, np.nan, np.inf, -np.inf], np.float32)
    lims_t, _, a_t = rorc.range_scan(base, query, is_empty, start, size, npl, thr)
    assert list(lims_t) == [0, 30, 30, 30, 30] and list(a_t) == live
    # a NaN query component: its segment is empty, the other segments are unchanged
    dirty = query.copy()
    dirty[0, 1] = np.nan
    lims_n, v_n, a_n = rorc.range_scan(base, dirty, is_empty, start, size, npl, -np.inf)
    assert list(lims_n) == [0, 30, 30, 45, 45]
    assert np.array_equal(a_n[:30], a[:30]) and np.array_equal(v_n[:30].view(np.uint32), v[:30].view(np.uint32))
    assert np.array_equal(a_n[30:], a[60:]) and np.array_equal(v_n[30:].view(np.uint32), v[60:].view(np.uint32))
    # without the tombstone mask
    lims_m, _, a_m = rorc.range_scan(base, query, None, start, size, npl, -np.inf)
    assert list(lims_m) == [0, 32, 64, 80, 80] and list(a_m[:32]) == list(range(16, 32)) + list(range(16))
