"""CPU: the surface of IVFPQIndex range search -- the six C-ABI symbols and their validation, the wrapper and the index
methods -- the range oracle (tests/ivfpq_range_oracle.py) pinned against float64 brute force where fp32 is exact, its
probe rules, and the conditions on the inputs of the GPU tests (tests/ivfpq_range_cases.py), asserted on the oracle
alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ivfpq_range_cases as cases
import ivfpq_range_oracle as rorc
from conftest import ROOT
from oracle import ivfpq_oracle as orc

RANGE_SYMBOLS = ("tpq_ivfpq_range_segments", "tpq_ivfpq_range_count", "tpq_ivfpq_range_fill",
                 "tpq_ivfpq_range_residual_segments", "tpq_ivfpq_range_residual_count",
                 "tpq_ivfpq_range_residual_fill")


def test_symbols_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in RANGE_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    assert lib.tpq_version() == 500
    assert lib.tpq_ivfpq_range_segments(7, 3) == 7 * 3 * 8
    assert lib.tpq_ivfpq_range_residual_segments(7, 5) == 7 * 5 * 8
    for nq, n_split in ((0, 1), (-1, 1), (5, 0), (5, 1025)):
        assert lib.tpq_ivfpq_range_segments(nq, n_split) == 0
    for nq, n_probe in ((0, 1), (-1, 1), (5, 0), (5, -2)):
        assert lib.tpq_ivfpq_range_residual_segments(nq, n_probe) == 0


def _entry_points():
    """(name, all-NULL arguments with a valid shape, the positions of n_slots / nq / max_nprobe / m / n_split)"""
    N_ = None
    #         codes lut query codebook ds metric empty start size npl thr counts n_slots nq np m  split stream
    count = [N_, N_, N_, N_, 2, 0, N_, N_, N_, N_, N_, N_, 100, 1, 4, 8, 1, N_]
    #        codes lut query codebook ds metric empty start size npl thr offs vals addr n_slots nq np m split stream
    fill = [N_, N_, N_, N_, 2, 0, N_, N_, N_, N_, N_, N_, N_, N_, 100, 1, 4, 8, 1, N_]
    #          codes part1 query codebook ds part2 full cells base empty start size npl thr counts n_slots nq np m stream
    rcount = [N_, N_, N_, N_, 2, N_, N_, N_, N_, N_, N_, N_, N_, N_, N_, 100, 1, 4, 8, N_]
    #         codes part1 query codebook ds part2 full cells base empty start size npl thr offs vals addr n_slots nq np m
    rfill = [N_, N_, N_, N_, 2, N_, N_, N_, N_, N_, N_, N_, N_, N_, N_, N_, N_, 100, 1, 4, 8, N_]
    return (("tpq_ivfpq_range_count", count, 12, True), ("tpq_ivfpq_range_fill", fill, 14, True),
            ("tpq_ivfpq_range_residual_count", rcount, 15, False), ("tpq_ivfpq_range_residual_fill", rfill, 17, False))


def test_arguments_are_checked_before_any_hip_call():
    """no GPU here: every rejection below happens before the library touches HIP"""
    from torchpq_amd import _lib
    lib = _lib.load()
    room = (C.c_char * 64)()                          # a non-NULL pointer nothing dereferences
    for name, args, n0, has_split in _entry_points():
        fn = getattr(lib, name)
        assert fn(*args) == -1 and "null pointer" in _lib.last_error(), name
        # m = 6 (not a multiple of 4), m = 0, max_nprobe = 0, nq = -1, n_slots = -1
        bad = [(n0 + 3, 6), (n0 + 3, 0), (n0 + 2, 0), (n0 + 1, -1), (n0, -1)]
        if has_split:
            bad += [(n0 + 4, 0), (n0 + 4, 1025)]
        for pos, value in bad:
            a = list(args)
            a[pos] = value
            assert fn(*a) == -1 and "null pointer" not in _lib.last_error(), (name, pos, value)
        a = list(args)
        a[n0] = (1 << 31) - 1
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
        a = list(args)
        a[n0 + 1] = 0
        assert fn(*a) == 0                             # no queries: nothing to do
        # every pointer given: m = 160 needs more LDS than a CU has; m = 156 with a long query does too
        full = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
        for m, ds in ((160, 1), (156, 8)):
            a = list(full)
            a[n0 + 3], a[4] = m, ds
            if name.startswith("tpq_ivfpq_range_residual"):
                a[1] = a[6] = None                     # part1 and full_lut absent: part1 is built from the query
            else:
                a[1] = None                            # lut absent: the table is built from the query
            assert fn(*a) == _lib.ERR_UNSUPPORTED and "LDS" in _lib.last_error(), (name, m, ds)
    # the plain form needs a table or (query, codebook); the residual form base_sims and one set of tables
    name, args, n0, _ = _entry_points()[0]
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[1] = a[2] = None
    assert getattr(lib, name)(*a) == -1 and "lut or (query, codebook)" in _lib.last_error()
    name, args, n0, _ = _entry_points()[2]
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[6] = a[5] = None
    assert getattr(lib, name)(*a) == -1 and "full_lut or" in _lib.last_error()
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[8] = None
    assert getattr(lib, name)(*a) == -1 and "base_sims" in _lib.last_error()


def test_wrapper_and_index_methods_exist():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    empty = inspect.Parameter.empty
    assert "IVFPQRangeHip" in kernels.__all__ and callable(kernels.IVFPQRangeHip)
    op = kernels.IVFPQRangeHip(m=8)
    assert op.last_n_split is None and callable(op.residual)
    sig = inspect.signature(index.IVFPQIndex.range_search)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("x", empty), ("threshold", empty), ("return_address", False), ("sort", False)]
    sig = inspect.signature(index.IVFPQIndex.range_search_cells)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("x", empty), ("cells", empty), ("threshold", empty), ("base_sims", None), ("n_probe_list", None),
        ("return_address", False), ("_extents", None)]
    doc = index.IVFPQIndex.range_search.__doc__
    assert "-squared-L2" in doc and "cosine similarity" in doc      # the threshold's value space is stated
    # both IVF indexes run the one batch loop
    from torchpq_amd.index import _range
    assert callable(_range.range_search_batches)
    for cls in (index.IVFPQIndex, index.IVFFlatIndex):
        assert "range_search_batches" in inspect.getsource(cls.range_search)


def test_ivfpqr_index_has_no_range_search():
    from torchpq_amd.index import IVFPQRIndex
    with pytest.raises(NotImplementedError, match="re-ranked"):
        IVFPQRIndex.range_search(None, torch.zeros(8, 1), -1.0)
    with pytest.raises(NotImplementedError, match="re-ranked"):
        IVFPQRIndex.range_search_cells(None, torch.zeros(8, 1), torch.zeros(1, 1, dtype=torch.long), -1.0)


def test_wrapper_declines_cpu_tensors_and_a_float64_threshold():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFPQRangeHip
    op = IVFPQRangeHip(m=8)
    data, lut = torch.zeros(2, 100, 4, dtype=torch.uint8), torch.zeros(8, 2, 256)
    cs, sz, npl = torch.zeros(2, 1, dtype=torch.long), torch.full((2, 1), 10), torch.ones(2, dtype=torch.long)
    base, part1, part2 = torch.zeros(2, 1), torch.zeros(2, 8, 256), torch.zeros(3, 8, 256)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op(data, cs, sz, npl, -1.0, precomputed=lut)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op(data, cs, sz, npl, torch.zeros(2), query=torch.zeros(16, 2), codebook=torch.zeros(8, 2, 256))
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op.residual(data, base, cs, sz, npl, -1.0, part1=part1, part2=part2, cells=cs)
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, torch.zeros(2, dtype=torch.float64), precomputed=lut)
    with pytest.raises(AssertionError):
        op.residual(data, base, cs, sz, npl, torch.zeros(2, dtype=torch.float64), part1=part1, part2=part2, cells=cs)
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, torch.zeros(3), precomputed=lut)           # one threshold per query
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, -1.0)                                      # neither a table nor (query, codebook)
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, -1.0, precomputed=lut.double())


# ---- the oracle against float64 brute force ---------------------------------------------------------------------
def _integer_index(seed, m, ds, n_cells, per_cell, nq):
    """small-integer codebooks, centroids and queries: every table entry and every partial sum is an integer far
    below 2^24, so fp32 is exact"""
    rng = np.random.default_rng(seed)
    cap = n_cells * per_cell
    codebook = rng.integers(-6, 7, (m, ds, 256)).astype(np.float32)
    centroids = rng.integers(-9, 10, (m * ds, n_cells)).astype(np.float32)
    query = rng.integers(-9, 10, (m * ds, nq)).astype(np.float32)
    storage = rng.integers(0, 256, (m // 4, cap, 4), dtype=np.uint8)
    sizes = rng.integers(per_cell // 2, per_cell + 1, n_cells).astype(np.int64)
    start = (np.arange(n_cells) * per_cell).astype(np.int64)
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    live = np.flatnonzero(is_empty == 0)
    storage[:, live[10:40]] = storage[:, live[5:6]]                      # thirty copies of one code: ties
    is_empty[rng.choice(live[40:], 30, replace=False)] = 1               # tombstones inside the cells
    cells = np.stack([rng.permutation(n_cells) for _ in range(nq)])      # every cell probed, in any order
    codes = orc.storage_to_codes(storage, np.arange(cap))
    decoded = orc.pq_decode(codebook, codes).astype(np.float64)          # [d, cap]
    cell_of = np.repeat(np.arange(n_cells), per_cell)
    return dict(codebook=codebook, centroids=centroids, query=query, storage=storage, sizes=sizes, start=start,
                is_empty=is_empty, cells=cells, decoded=decoded, cell_of=cell_of, cap=cap,
                npl=np.full(nq, n_cells, np.int64))


def _check_hit_sets(ix, exact, got, thr):
    lims, v, a = got
    live = np.flatnonzero(ix["is_empty"] == 0)
    assert np.abs(exact).max() < 2 ** 24
    for q in range(exact.shape[0]):
        want = live[exact[q, live] >= float(thr[q])]
        seg = slice(lims[q], lims[q + 1])
        assert len(want) > 0 and np.array_equal(np.sort(a[seg]), want)   # every cell is probed: the hit SET is exact
        assert np.array_equal(v[seg].astype(np.float64), exact[q, a[seg]])
        # scan order: probe rank ascending, then address ascending
        rank = np.argsort(ix["cells"][q])[ix["cell_of"][a[seg]]]
        assert np.array_equal(np.lexsort((a[seg], rank)), np.arange(len(want)))


@pytest.mark.parametrize("metric", ["euclidean", "inner"])
def test_oracle_equals_float64_brute_force_on_integer_data(metric):
    """plain PQ with every cell probed: the hit set of range_scan is {i live : value(i) >= thr} in float64, value(i) =
    -|q - decode(i)|^2 or q . decode(i).  Query 0's threshold lies on the value of thirty equal codes: inclusive."""
    ix = _integer_index(5, m=8, ds=2, n_cells=6, per_cell=70, nq=5)
    q64 = ix["query"].astype(np.float64)
    if metric == "euclidean":
        exact = np.stack([-((q64[:, q:q + 1] - ix["decoded"]) ** 2).sum(0) for q in range(5)])
    else:
        exact = np.stack([(q64[:, q:q + 1] * ix["decoded"]).sum(0) for q in range(5)])
    live = np.flatnonzero(ix["is_empty"] == 0)
    thr = np.array([np.sort(exact[q, live])[len(live) // 2] for q in range(5)], np.float32)
    thr[0] = exact[0, live[5]]
    lut = orc.adc_lut(ix["query"], ix["codebook"], metric)
    got = rorc.range_scan(ix["storage"], lut, ix["is_empty"], ix["start"][ix["cells"]], ix["sizes"][ix["cells"]],
                          ix["npl"], thr)
    _check_hit_sets(ix, exact, got, thr)
    assert np.isin(live[10:40], got[2][got[0][0]:got[0][1]]).all()      # on the threshold: all thirty are hits
    up = rorc.range_scan(ix["storage"], lut, ix["is_empty"], ix["start"][ix["cells"]], ix["sizes"][ix["cells"]],
                         ix["npl"], np.nextafter(thr, np.float32(np.inf)))
    assert not np.isin(live[10:40], up[2][up[0][0]:up[0][1]]).any()     # one ulp above: none of them


@pytest.mark.parametrize("tables", ["parts", "full"])
def test_residual_oracle_equals_float64_brute_force_on_integer_data(tables):
    """residual PQ: decode(i) = centroid(cell of i) + decoded residual, base_sims = -|q - c|^2, part1 = 2 q . r, part2 =
    -2 c . r - |r|^2: the value is -|q - decode(i)|^2 exactly"""
    ix = _integer_index(6, m=8, ds=2, n_cells=6, per_cell=70, nq=5)
    q64, c64 = ix["query"].astype(np.float64), ix["centroids"].astype(np.float64)
    full_vec = c64[:, ix["cell_of"]] + ix["decoded"]
    exact = np.stack([-((q64[:, q:q + 1] - full_vec) ** 2).sum(0) for q in range(5)])
    live = np.flatnonzero(ix["is_empty"] == 0)
    thr = np.array([np.sort(exact[q, live])[(2 * len(live)) // 3] for q in range(5)], np.float32)
    base = np.stack([-((q64[:, q:q + 1] - c64[:, ix["cells"][q]]) ** 2).sum(0) for q in range(5)]).astype(np.float32)
    part1 = orc.residual_part1(ix["query"], ix["codebook"])
    part2 = orc.residual_part2(ix["centroids"], ix["codebook"])
    full = None
    if tables == "full":
        full = (part1[:, None] + part2[ix["cells"]]).astype(np.float32)   # [nq, n_probe, m, 256]
        part1 = part2 = None
    got = rorc.range_scan_residual(ix["storage"], part1, part2, ix["cells"], base, ix["is_empty"],
                                   ix["start"][ix["cells"]], ix["sizes"][ix["cells"]], ix["npl"], thr, full=full)
    _check_hit_sets(ix, exact, got, thr)


def test_oracle_probe_rules_thresholds_and_nan():
    m, cap = 4, 64
    rng = np.random.default_rng(0)
    storage = rng.integers(0, 256, (1, cap, 4), dtype=np.uint8)
    lut = rng.standard_normal((m, 4, 256)).astype(np.float32)
    start = np.array([[16, 16, 0, 56]] * 4, np.int64)     # the second probe repeats the first: skipped
    size = np.array([[16, 16, 16, 20]] * 4, np.int64)     # the fourth cell leaves the storage: cut at slot 64
    is_empty = np.zeros(cap, np.uint8)
    is_empty[[3, 22, 60]] = 1
    npl = np.array([9, 4, 3, 0], np.int64)                # clamped to [0, 4]
    live = ([s for s in range(16, 32) if s != 22] + [s for s in range(16) if s != 3]
            + [s for s in range(56, 64) if s != 60])      # probe rank, then address
    lims, v, a = rorc.range_scan(storage, lut, is_empty, start, size, npl, -np.inf)
    assert list(lims) == [0, 37, 74, 104, 104]
    assert list(a[:37]) == live and list(a[37:74]) == live and list(a[74:]) == live[:30]
    assert np.array_equal(v[:37].view(np.uint32), orc.scan_values(storage, lut[:, 0], np.array(live)).view(np.uint32))
    # +inf and NaN thresholds: nothing; per-query thresholds are per query
    for t in (np.inf, np.nan):
        lims_t, v_t, a_t = rorc.range_scan(storage, lut, is_empty, start, size, npl, t)
        assert list(lims_t) == [0] * 5 and len(v_t) == len(a_t) == 0
    thr = np.array([-np.inf, np.nan, np.inf, -np.inf], np.float32)
    lims_t, _, a_t = rorc.range_scan(storage, lut, is_empty, start, size, npl, thr)
    assert list(lims_t) == [0, 37, 37, 37, 37] and list(a_t) == live
    # a NaN table (a NaN query component): its segment is empty, the other segments are unchanged
    dirty = lut.copy()
    dirty[2, 1] = np.nan
    lims_n, v_n, a_n = rorc.range_scan(storage, dirty, is_empty, start, size, npl, -np.inf)
    assert list(lims_n) == [0, 37, 37, 67, 67]
    assert np.array_equal(a_n[37:], a[74:]) and np.array_equal(v_n[37:].view(np.uint32), v[74:].view(np.uint32))
    # without the tombstone mask; a negative size is an empty cell
    size[:, 2] = -3
    lims_m, _, a_m = rorc.range_scan(storage, lut, None, start, size, npl, -np.inf)
    assert list(lims_m) == [0, 24, 48, 64, 64] and list(a_m[:24]) == list(range(16, 32)) + list(range(56, 64))
    # the residual form walks the same probes: rank 1 is skipped, its base_sims and cell never used
    part1 = rng.standard_normal((4, m, 256)).astype(np.float32)
    part2 = rng.standard_normal((3, m, 256)).astype(np.float32)
    cells = np.array([[1, 1, 0, 2]] * 4, np.int64)
    base = rng.standard_normal((4, 4)).astype(np.float32)
    size[:, 2] = 16
    lims_r, v_r, a_r = rorc.range_scan_residual(storage, part1, part2, cells, base, is_empty, start, size, npl, -np.inf)
    assert list(lims_r) == [0, 37, 74, 104, 104] and list(a_r[:37]) == live
    lut_p = (part1[0] + part2[0]).astype(np.float32)                     # query 0, probe rank 2: cell 0
    want = np.full(1, base[0, 2], np.float32)
    for j in range(m):
        want = (want + lut_p[j, storage[0, 0, j]]).astype(np.float32)
    assert v_r[15].view(np.uint32) == want[0].view(np.uint32) and a_r[15] == 0
    sv, sa = rorc.sort_segments(lims, v, a)
    for q in range(4):
        seg = slice(lims[q], lims[q + 1])
        assert np.array_equal(np.lexsort((sa[seg], -sv[seg].astype(np.float64))), np.arange(lims[q + 1] - lims[q]))
        assert sorted(sa[seg]) == sorted(a[seg])


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------
def _layout_is_what_the_gpu_tests_claim(case, nq, n_probe):
    cap = case["storage"].shape[1]
    over = (case["cs"] + case["sz"] > cap)
    assert over[0].any()                                                 # query 0 probes the cell that leaves the storage
    assert (case["is_empty"][[s for s, _ in case["cand"]][0]] == 0).all() and case["is_empty"].sum() > 25
    assert set(np.unique(case["sz"])) <= set(cases.CELL_SIZES) | {cases.OVER_SIZE}
    if nq > 1 and n_probe > 1:
        assert case["cs"][1, 1] == case["cs"][1, 0]                      # one cell listed twice in a row
    if nq >= 3:
        assert case["npl"][-1] == 0 and case["n_cand"][-1] == 0
    if nq >= 100:
        assert (case["npl"] > n_probe).any() and (case["npl"] < n_probe).any() and (case["npl"] == n_probe).any()
    for s, v in case["cand"]:
        assert s.size == 0 or (s.min() >= 0 and s.max() < cap)
    # duplicate codes: values repeat, so thresholds taken from the values sit on ties
    s0, v0 = case["cand"][0]
    assert len(np.unique(v0)) < len(v0)


@pytest.mark.parametrize("m,ds,table,nq,n_probe,metric", cases.PLAIN_CASES)
def test_gpu_plain_cases_are_not_vacuous(m, ds, table, nq, n_probe, metric):
    case = cases.plain_case(m, ds, table, nq, n_probe, metric)
    cases.assert_not_vacuous(case, nq)
    _layout_is_what_the_gpu_tests_claim(case, nq, n_probe)
    assert case["lut"].shape == (m, nq, 256) and np.isfinite(case["lut"]).all()


@pytest.mark.parametrize("m,ds,tables,nq,n_probe", cases.RESIDUAL_CASES)
def test_gpu_residual_cases_are_not_vacuous(m, ds, tables, nq, n_probe):
    case = cases.residual_case(m, ds, tables, nq, n_probe)
    cases.assert_not_vacuous(case, nq)
    _layout_is_what_the_gpu_tests_claim(case, nq, n_probe)
    assert (case["full"] is not None) == (tables == "full")
