"""CPU: the surface of IVFPQ4Index range search -- the six C-ABI symbols and their validation, the wrapper and the index
methods --, the range oracle (tests/ivfpq4_range_oracle.py) against the top-k oracles where they must agree, and the
conditions on the inputs of the GPU tests (tests/ivfpq4_range_cases.py), asserted on the oracle alone."""
import ctypes as C
import inspect
import os
import re
import sys

import numpy as np
import pytest
import torch

import ivfpq4_range_cases as cases
import ivfpq4_range_guarded as guarded
import ivfpq4_range_oracle as rgo
from conftest import ROOT

COUNT, FILL = "tpq_ivfpq4_range_count", "tpq_ivfpq4_range_fill"
RCOUNT, RFILL = "tpq_ivfpq4_range_residual_count", "tpq_ivfpq4_range_residual_fill"
SEGMENTS, RSEGMENTS = "tpq_ivfpq4_range_segments", "tpq_ivfpq4_range_residual_segments"


def test_symbols_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    lib = _lib.load()
    for name in (COUNT, FILL, RCOUNT, RFILL, SEGMENTS, RSEGMENTS):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert re.search(r"#define\s+TPQ_HAS_IVFPQ4_RANGE\s+1\b", header)
    for name in (SEGMENTS, RSEGMENTS):
        assert _lib.SIGNATURES[name] == (C.c_size_t, [C.c_int, C.c_int])
    res, args = _lib.SIGNATURES[COUNT]
    assert res is C.c_int and len(args) == 21 and args[9] is C.c_int and args[10] is C.c_int64 and args[13] is C.c_int64
    res, args = _lib.SIGNATURES[FILL]
    assert res is C.c_int and len(args) == 23 and args[9] is C.c_int and args[10] is C.c_int64 and args[15] is C.c_int64
    res, args = _lib.SIGNATURES[RCOUNT]
    assert res is C.c_int and len(args) == 23 and args[5] is C.c_int and args[12] is C.c_int and args[13] is C.c_int64
    assert args[16] is C.c_int64
    res, args = _lib.SIGNATURES[RFILL]
    assert res is C.c_int and len(args) == 25 and args[5] is C.c_int and args[12] is C.c_int and args[13] is C.c_int64
    assert args[18] is C.c_int64
    # the arguments of the declarations, counted in the header itself
    for name, n in ((COUNT, 21), (FILL, 23), (RCOUNT, 23), (RFILL, 25)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % name, header).group(1)
        assert decl.count(",") + 1 == n, name


def test_segment_functions():
    from torchpq_amd import _lib
    lib = _lib.load()
    assert lib.tpq_ivfpq4_range_segments(3, 5) == 3 * 5 * 8 and lib.tpq_ivfpq4_range_segments(1, 1024) == 8 * 1024
    for nq, n_split in ((0, 1), (-1, 1), (1, 0), (1, 1025), (1, -3)):
        assert lib.tpq_ivfpq4_range_segments(nq, n_split) == 0
    assert lib.tpq_ivfpq4_range_residual_segments(3, 4) == 3 * 4 * 8
    assert lib.tpq_ivfpq4_range_residual_segments(7, 2000) == 7 * 2000 * 8
    for nq, n_probe in ((0, 1), (-1, 1), (1, 0), (1, -1)):
        assert lib.tpq_ivfpq4_range_residual_segments(nq, n_probe) == 0


def _entry_points():
    """(name, all-NULL arguments with a valid shape, the position of n_filters -- filter_stride follows it --, the
    position of n_slots -- m, ds, nq, max_nprobe, metric (and n_split) follow it --, has n_split)"""
    N_ = None
    #  codes query codebook empty start size npl bits ofq nf stride thr counts n_slots m ds nq np metric split stream
    count = [N_, N_, N_, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, 100, 8, 2, 1, 4, 0, 1, N_]
    fill = [N_, N_, N_, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, N_, N_, 100, 8, 2, 1, 4, 0, 1, N_]
    #  codes query codebook centroids cells n_cells empty start size npl bits ofq nf stride thr counts n_slots ...
    rcount = [N_, N_, N_, N_, N_, 3, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, 100, 8, 2, 1, 4, 0, N_]
    rfill = [N_, N_, N_, N_, N_, 3, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, N_, N_, 100, 8, 2, 1, 4, 0, N_]
    return ((COUNT, count, 9, 13, True), (FILL, fill, 9, 15, True), (RCOUNT, rcount, 12, 16, False),
            (RFILL, rfill, 12, 18, False))


def test_arguments_are_checked_before_any_hip_call():
    """no GPU here: every rejection below happens before the library touches HIP"""
    from torchpq_amd import _lib
    lib = _lib.load()
    room = (C.c_char * 64)()                          # a non-NULL pointer nothing dereferences
    for name, args, nf, n0, has_split in _entry_points():
        fn = getattr(lib, name)
        M, DS, NQ, NP, METRIC, SPLIT = (n0 + i for i in range(1, 7))

        def call(**changes):
            a = list(args)
            for pos, value in changes.items():
                a[int(pos[1:])] = value
            return fn(*a)
        at = lambda pos, value: call(**{"p%d" % pos: value})
        assert fn(*args) == -1 and "null pointer" in _lib.last_error(), name
        for m in (12, 4, 0, 264):                      # no multiple of 8, below 8, above 256
            assert at(M, m) == _lib.ERR_UNSUPPORTED and "m must be a multiple of 8" in _lib.last_error(), (name, m)
        assert at(DS, 0) == _lib.ERR_UNSUPPORTED
        if has_split:
            for n_split in (0, 1025):
                assert at(SPLIT, n_split) == -1 and "n_split" in _lib.last_error(), (name, n_split)
        assert at(METRIC, 7) == -1 and "metric" in _lib.last_error()
        assert at(NP, 0) == -1 and at(NQ, -1) == -1 and at(n0, -1) == -1
        assert at(n0, (1 << 31) - 1) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
        assert at(NQ, 0) == 0                          # no queries: nothing to do
        # without filter_bits the other filter arguments are not looked at
        assert call(**{"p%d" % nf: 0, "p%d" % (nf + 1): 0}) == -1 and "null pointer" in _lib.last_error()
        # with filter_bits: n_filters >= 1, filter_stride >= ceil(n_slots / 32)
        bits = {"p%d" % (nf - 2): C.addressof(room)}
        for n_filters in (0, -2):
            assert call(**bits, **{"p%d" % nf: n_filters}) == -1 and "n_filters" in _lib.last_error(), (name, n_filters)
        assert call(**bits, **{"p%d" % (nf + 1): 3}) == -1 and "filter_stride" in _lib.last_error()   # one word short
        assert call(**bits) == -1 and "null pointer" in _lib.last_error()
        assert call(**bits, **{"p%d" % NQ: 0}) == 0
        # every pointer given but one: each of the required ones is missed, the optional ones are not
        full = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
        optional = {3 if nf == 9 else 6, nf - 2, nf - 1}         # is_empty, filter_bits, filter_of_query
        for pos, v in enumerate(args[:-1]):
            if v is not None or pos in optional:
                continue
            a = list(full)
            a[pos] = None
            assert fn(*a) == -1 and "null pointer" in _lib.last_error(), (name, pos)
        # m = 256 with sub-vectors of 160 floats: the staged query alone is 160 KiB
        a = list(full)
        a[M], a[DS] = 256, 160
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "LDS" in _lib.last_error(), name
        a[DS] = 1 << 13                                # d beyond anything: declined before the LDS is sized
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "m * ds" in _lib.last_error(), name
    for name, args, nf, n0, _ in _entry_points()[2:]:
        a = list(args)
        a[5] = 0
        assert getattr(lib, name)(*a) == -1 and "n_cells" in _lib.last_error()


def test_wrapper_and_index_methods_exist():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    empty = inspect.Parameter.empty
    params = lambda fn: [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
    assert "IVFPQ4RangeHip" in kernels.__all__ and callable(kernels.IVFPQ4RangeHip)
    op = kernels.IVFPQ4RangeHip(m=8)
    assert op.last_n_split is None and callable(op.residual)
    assert kernels.IVFPQ4RangeHip._n_split is kernels.IVFFlatTopkHip._n_split
    for bad in (4, 12, 264):
        with pytest.raises(AssertionError):
            kernels.IVFPQ4RangeHip(m=bad)
    assert params(op.__call__.__func__) == [
        ("codes", empty), ("query", empty), ("codebook", empty), ("cell_start", empty), ("cell_size", empty),
        ("n_probe_list", empty), ("threshold", empty), ("filter_bits", None), ("filter_of_query", None),
        ("is_empty", None), ("distance", "euclidean"), ("n_split", None), ("slots_hint", None)]
    assert [n for n, _ in params(op.residual.__func__)] == [
        "codes", "query", "codebook", "centroids", "cells", "cell_start", "cell_size", "n_probe_list", "threshold",
        "filter_bits", "filter_of_query", "is_empty", "distance"]
    I4, IF = index.IVFPQ4Index, index.IVFFlatIndex
    for method in ("range_search", "range_search_filtered"):
        assert params(getattr(I4, method)) == params(getattr(IF, method)), method
    assert params(I4.range_search_cells) == params(index.IVFPQIndex.range_search_cells)
    assert params(I4.range_search_cells_filtered) == [
        ("x", empty), ("cells", empty), ("threshold", empty), ("flt", empty), ("filter_of_query", None),
        ("base_sims", None), ("n_probe_list", None), ("return_address", False), ("_extents", None)]
    doc = sys.modules[I4.__module__].__doc__
    assert "range_search" in doc and "No range search" not in doc


def test_wrapper_declines_cpu_tensors_and_bad_arguments():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFPQ4RangeHip
    op = IVFPQ4RangeHip(m=8)
    codes, query, codebook = torch.zeros(1, 100, 4, dtype=torch.uint8), torch.zeros(16, 2), torch.zeros(8, 2, 16)
    cs, sz, npl = torch.zeros(2, 1, dtype=torch.long), torch.full((2, 1), 10), torch.ones(2, dtype=torch.long)
    centroids = torch.zeros(3, 16)
    bits, rows = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    plain = lambda *a, **kw: op(codes, query, codebook, cs, sz, npl, *a, **kw)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        plain(0.0)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        plain(torch.zeros(2), bits, rows)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op.residual(codes, query, codebook, centroids, cs, cs, sz, npl, 0.0, bits)
    with pytest.raises(AssertionError):
        plain(torch.zeros(3))                                              # one threshold per query
    with pytest.raises(AssertionError):
        plain(torch.zeros(2, dtype=torch.float64))
    with pytest.raises(AssertionError):
        plain(0.0, bits[:, :3])                                            # a row one word short of the storage
    with pytest.raises(AssertionError):
        plain(0.0, bits, rows.long())                                      # int32 at the C ABI
    with pytest.raises(AssertionError):
        plain(0.0, None, rows)                                             # rows without a filter
    with pytest.raises(AssertionError):
        op.residual(codes, query, codebook, centroids[:, :-1], cs, cs, sz, npl, 0.0)       # another d
    with pytest.raises(AssertionError):
        op.residual(codes, query, codebook, centroids, cs[:1], cs, sz, npl, 0.0)           # cells of another batch


# ---- the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", [k for k in cases.KERNEL_CASES if k[2] <= 3])
def test_oracle_at_minus_inf_sorted_is_the_topk_oracle_at_full_depth(m, ds, nq, n_probe, distance, residual):
    """plain, residual and filtered: every run of the case against ivfpq4_filtered_cases' full-depth lists (the
    unfiltered top-k oracles under `is_empty | ~allowed_row`; the last run is row 0, all ones: the unfiltered scan)"""
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    for run in list(range(len(c["runs"]))) + [None]:
        cand = cases.candidates(c, residual, distance, run=run)
        lims, v, a = rgo.hits(cand, -np.inf)
        sv, sa = rgo.sort_segments(lims, v, a)
        fv, fa = c["full"][len(c["runs"]) - 1 if run is None else run]
        for q in range(nq):
            n = int((fa[q] >= 0).sum())
            assert lims[q + 1] - lims[q] == n
            assert np.array_equal(sa[lims[q]:lims[q + 1]], fa[q, :n])
            assert np.array_equal(sv[lims[q]:lims[q + 1]].view(np.uint32), fv[q, :n].view(np.uint32))
        assert len(a) > 0 or run is not None


def test_oracle_threshold_rules():
    c = cases.case(8, 2, 3, 8, "inner", False)
    cand = cases.candidates(c, False, "inner")
    n = [len(s) for s, _ in cand]
    assert rgo.hits(cand, np.inf)[0].tolist() == [0, 0, 0, 0] and rgo.hits(cand, np.nan)[0].tolist() == [0, 0, 0, 0]
    assert np.array_equal(np.diff(rgo.hits(cand, -np.inf)[0]), n)
    lims, v, a = rgo.hits(cand, np.array([-np.inf, np.nan, np.inf], np.float32))
    assert lims.tolist() == [0, n[0], n[0], n[0]] and np.array_equal(a, cand[0][0])
    # a row outside the filter allows nothing
    out = rgo.candidates(c["storage"], c["query"], c["codebook"], c["is_empty"], c["cs"], c["sz"], c["npl"], "inner",
                         allowed=c["allowed"], rows=np.array([0, -1, len(cases.ROWS)], np.int32))
    assert np.array_equal(out[0][0], cand[0][0]) and len(out[1][0]) == len(out[2][0]) == 0


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", cases.KERNEL_CASES)
def test_gpu_cases_are_not_vacuous(m, ds, nq, n_probe, distance, residual):
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    assert c["storage"].shape[1] % 32 != 0
    cand = cases.candidates(c, residual, distance)
    thr = cases.thresholds(cand)
    assert cases.boundary_exists(cand, thr)                               # the boundary candidate exists ...
    b, ab = rgo.hits(cand, thr["boundary"])[0], rgo.hits(cand, thr["above"])[0]
    assert (np.diff(b) >= np.diff(ab)).all() and (np.diff(b) > np.diff(ab)).any()   # ... and the next float up loses it
    n = np.array([int((~np.isnan(v)).sum()) for _, v in cand])
    none = all_of = partly = False
    for name, t in thr.items():
        got = np.diff(rgo.hits(cand, t)[0])
        none |= bool((got == 0).any())                                    # some query has no hit
        all_of |= bool(((got == n) & (n > 0)).any())                      # some has all its candidates
        partly |= bool(((got > 0) & (got < n)).any())
    assert none and all_of and partly
    if nq > 1:
        special = np.concatenate([t for name, t in thr.items() if name.startswith("mixed")])
        assert np.isnan(special).any() and np.isposinf(special).any() and np.isneginf(special).any()
    else:
        assert np.isnan(thr["nan"]).all() and np.isposinf(thr["plus_inf"]).all() and np.isneginf(thr["minus_inf"]).all()
    if nq > 3:
        return
    # some segment of a wave is empty next to a full one
    cand_p = cases.candidates(c, residual, distance, probes=True)
    seen = False
    for n_split in ((1,) if residual else (1, 5)):
        counts = cases.segment_counts(c, cand_p, thr["median"], residual, n_split)
        assert counts.sum() == rgo.hits(cand, thr["median"])[0][-1]
        seen |= bool(((counts == 0).any(2) & (counts > 0).any(2)).any())
    assert seen
    # the sparse row empties a tile of the 300-slot cell next to a tile with hits, for some query at -inf
    start, sparse = c["big_start"], c["allowed"][3] & (c["is_empty"] == 0)
    tiles = [sparse[start + 64 * t:start + 64 * t + 64].any() for t in range(5)]
    assert not tiles[1] and tiles[0]
    hit_big = False
    for run, rows in enumerate(c["runs"][:-1]):
        for q, (s, _) in enumerate(cases.candidates(c, residual, distance, run=run)):
            if rows[q] == 3 and ((s >= start) & (s < start + 64)).any():
                hit_big = True
                assert not ((s >= start + 64) & (s < start + 128)).any()
    assert hit_big


def test_overlap_case_scans_sixty_slots_twice():
    c = cases.overlap_case()
    p, s = __import__("ivfpq4_residual_oracle").probe_slots(c["cs"][0], c["sz"][0], c["npl"][0], c["storage"].shape[1])
    assert len(np.intersect1d(s[p == 0], s[p == 1])) == 60 and c["cells"][0, 0] != c["cells"][0, 1]
    live = c["is_empty"][s] == 0
    assert len(np.intersect1d(s[(p == 0) & live], s[(p == 1) & live])) > 20
    assert not np.array_equal(c["centroids"][1], c["centroids"][2])


def test_the_four_launching_entry_points_have_a_guarded_case():
    """the table of tests/guarded_cases.py holds a case for each new launching entry point, with a builder in
    tests/test_gpu_guarded_buffers.BUILDERS (registered by tests/ivfpq4_range_guarded.py)"""
    import guarded_cases
    import test_gpu_guarded_buffers as gpu
    for cid, symbols in guarded.CASE_SYMBOLS.items():
        assert guarded_cases.CASE_SYMBOLS[cid] == symbols and guarded_cases.CASE_IDS.count(cid) == 1
        assert callable(gpu.BUILDERS[cid]) and cid not in guarded_cases.NOT_BIT_EXACT
        for s in symbols:
            assert guarded_cases.CASES[s] == [cid]
    assert {COUNT, FILL, RCOUNT, RFILL} == {s for symbols in guarded.CASE_SYMBOLS.values() for s in symbols}
    guarded.register()                                                   # (a second registration changes nothing)
    assert len(guarded_cases.CASE_IDS) == len(set(guarded_cases.CASE_IDS)) == len(gpu.BUILDERS)
