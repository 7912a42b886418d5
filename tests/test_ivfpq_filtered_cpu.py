"""CPU: the surface of IVFPQIndex filtered search -- the four C-ABI symbols and their validation, the wrapper and the
index methods -- the filtered oracle (tests/ivfpq_filtered_oracle.py) against the top-k oracle where they must agree,
and the conditions on the inputs of the GPU tests (tests/ivfpq_filtered_cases.py), asserted on the oracle alone."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ivfpq_filtered_cases as cases
import ivfpq_filtered_oracle as forc
from conftest import ROOT
from oracle import ivfpq_oracle as orc

SYMBOLS = ("tpq_ivfpq_scan_filtered_workspace_bytes", "tpq_ivfpq_scan_filtered_topk",
           "tpq_ivfpq_scan_filtered_residual_topk", "tpq_slot_filter_build")


def test_symbols_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
    lib = _lib.load()
    ws = lib.tpq_ivfpq_scan_filtered_workspace_bytes
    assert ws(7, 100, 1) == 0                                  # a query that is one workgroup needs no lists
    assert ws(7, 100, 3) == 7 * 3 * 128 * 8 and ws(7, 1000, 3) == 7 * 3 * 1024 * 8 and ws(7, 1, 2) == 7 * 2 * 64 * 8
    for nq, k, n_split in ((0, 10, 2), (-1, 10, 2), (5, 0, 2), (5, 1025, 2), (5, 10, 0), (5, 10, 1025)):
        assert ws(nq, k, n_split) == 0


def _entry_points():
    """(name, all-NULL arguments with a valid shape, the position of n_filters, the position of n_slots -- nq,
    max_nprobe, m and k follow it --, has n_split)"""
    N_ = None
    #        codes lut query codebook ds metric empty start size npl bits ofq nf stride vals addr a2i ids n_slots nq np m
    plain = [N_, N_, N_, N_, 2, 0, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, N_, N_, 100, 1, 4, 8, 10, 1, N_, 0, N_]
    #      codes part1 query codebook ds part2 full cells base empty start size npl bits ofq nf stride vals addr a2i ids
    res = [N_, N_, N_, N_, 2, N_, N_, N_, N_, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, N_, N_, 100, 1, 4, 8, 10, N_]
    return (("tpq_ivfpq_scan_filtered_topk", plain, 12, 18, True),
            ("tpq_ivfpq_scan_filtered_residual_topk", res, 15, 21, False))


def test_arguments_are_checked_before_any_hip_call():
    """no GPU here: every rejection below happens before the library touches HIP"""
    from torchpq_amd import _lib
    lib = _lib.load()
    room = (C.c_char * 64)()                          # a non-NULL pointer nothing dereferences
    for name, args, nf, n0, has_split in _entry_points():
        fn = getattr(lib, name)
        assert fn(*args) == -1 and "null pointer" in _lib.last_error(), name
        # m = 6 (not a multiple of 4), m = 0, max_nprobe = 0, nq = -1, n_slots = -1, k = 0, k = 1025, no filter row,
        # a stride one word short of ceil(100 / 32) = 4
        bad = [(n0 + 3, 6), (n0 + 3, 0), (n0 + 2, 0), (n0 + 1, -1), (n0, -1), (n0 + 4, 0), (n0 + 4, 1025), (nf, 0),
               (nf + 1, 3)]
        if has_split:
            bad += [(n0 + 5, 0), (n0 + 5, 1025)]
        for pos, value in bad:
            a = list(args)
            a[pos] = value
            assert fn(*a) == -1 and "null pointer" not in _lib.last_error(), (name, pos, value)
        a = list(args)
        a[nf + 1] = 3
        assert fn(*a) == -1 and "filter_stride" in _lib.last_error()
        a = list(args)
        a[n0 + 4] = 1025
        assert fn(*a) == -1 and "k=1025" in _lib.last_error()
        a = list(args)
        a[n0], a[nf + 1] = (1 << 31) - 1, 1 << 26
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
        # the largest m is cases.MAX_M: one row word more does not fit the LDS beside the queues and the pending lists
        a = list(args)
        a[n0 + 3] = cases.MAX_M + 4
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "LDS" in _lib.last_error(), name
        a = list(args)
        a[n0 + 1] = 0
        assert fn(*a) == 0                             # no queries: nothing to do
        # every pointer given: the largest m with a long staged query needs more LDS than a CU has
        full = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
        a = list(full)
        a[n0 + 3], a[4] = cases.MAX_M, 16
        if has_split:
            a[1] = None                                # lut absent: the table is built from the query
        else:
            a[1] = a[6] = None                         # part1 and full_lut absent: part1 is built from the query
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "LDS" in _lib.last_error(), name
        # out_ids only together with address2id
        a = list(full)
        a[nf + 4] = None
        assert fn(*a) == -1 and "address2id" in _lib.last_error()
    # the plain form needs a table or (query, codebook) and, split, a workspace
    name, args, nf, n0, _ = _entry_points()[0]
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[1] = a[2] = None
    assert getattr(lib, name)(*a) == -1 and "lut or (query, codebook)" in _lib.last_error()
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[n0 + 5], a[n0 + 6], a[n0 + 7] = 2, None, 0
    assert getattr(lib, name)(*a) == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    # the residual form base_sims and one set of tables
    name, args, nf, n0, _ = _entry_points()[1]
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[6] = a[5] = None
    assert getattr(lib, name)(*a) == -1 and "full_lut or" in _lib.last_error()
    a = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    a[8] = None
    assert getattr(lib, name)(*a) == -1 and "base_sims" in _lib.last_error()
    # the bits
    build = lib.tpq_slot_filter_build
    assert build(None, 5, None, 100, None) == -1 and "null pointer" in _lib.last_error()
    assert build(None, -1, None, 100, None) == -1 and build(None, 5, None, -1, None) == -1
    assert build(None, 0, None, 100, None) == 0 and build(None, 5, None, 0, None) == 0
    assert build(None, 5, None, (1 << 31) - 1, None) == _lib.ERR_UNSUPPORTED


def test_wrapper_and_index_methods_exist():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    from torchpq_amd.index import _coarse, _filter
    empty = inspect.Parameter.empty
    assert "IVFPQFilteredTopkHip" in kernels.__all__ and callable(kernels.IVFPQFilteredTopkHip)
    op = kernels.IVFPQFilteredTopkHip(m=8)
    assert op.last_n_split is None and callable(op.residual)
    assert kernels.IVFPQFilteredTopkHip._n_split is kernels.IVFPQTopkHip._n_split
    sig = inspect.signature(index.IVFPQIndex.search_filtered)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [
        ("x", empty), ("k", empty), ("flt", empty), ("filter_of_query", None)]
    sig = inspect.signature(index.IVFPQIndex.search_cells_filtered)
    assert [p.name for p in list(sig.parameters.values())[1:4]] == ["x", "cells", "flt"]
    assert sig.parameters["return_address"].default is False
    assert callable(index.IVFPQIndex.id_filter) and callable(_filter.IdFilter)
    # the batch loop cuts per-query tensors alongside the queries, and existing callers get what they got
    sig = inspect.signature(_coarse.CoarseProbeMixin._search_batches)
    assert list(sig.parameters)[1:3] == ["x", "per_batch"] and sig.parameters["alongside"].default == ()


def test_ivfpqr_index_has_no_filtered_search():
    from torchpq_amd.index import IVFPQRIndex
    with pytest.raises(NotImplementedError, match="re-ranked"):
        IVFPQRIndex.search_filtered(None, torch.zeros(8, 1), 1, None)
    with pytest.raises(NotImplementedError, match="re-ranked"):
        IVFPQRIndex.search_cells_filtered(None, torch.zeros(8, 1), torch.zeros(1, 1, dtype=torch.long), None)


def test_wrapper_declines_cpu_tensors_and_bad_filters():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFPQFilteredTopkHip, SlotFilterBuildHip
    op = IVFPQFilteredTopkHip(m=8)
    data, lut = torch.zeros(2, 100, 4, dtype=torch.uint8), torch.zeros(8, 2, 256)
    cs, sz, npl = torch.zeros(2, 1, dtype=torch.long), torch.full((2, 1), 10), torch.ones(2, dtype=torch.long)
    base, part1, part2 = torch.zeros(2, 1), torch.zeros(2, 8, 256), torch.zeros(3, 8, 256)
    bits, rows = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op(data, cs, sz, npl, 5, bits, rows, precomputed=lut)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op.residual(data, base, cs, sz, npl, 5, bits, part1=part1, part2=part2, cells=cs)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        SlotFilterBuildHip()(torch.zeros(3, dtype=torch.long), bits[0], 100)
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, 5, bits[:, :3], precomputed=lut)            # a row one word short of the storage
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, 5, bits.long(), precomputed=lut)
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, 5, bits, rows.long(), precomputed=lut)      # int32 at the C ABI
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, 5, bits, rows[:1], precomputed=lut)         # one row per query
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, 1025, bits, precomputed=lut)
    with pytest.raises(AssertionError):
        op(data, cs, sz, npl, 5, bits)                                    # neither a table nor (query, codebook)


# ---- the oracle ---------------------------------------------------------------------------------------------------
def test_bit_packing_round_trip_and_build():
    rng = np.random.default_rng(0)
    allowed = rng.random((3, 77)) < 0.4
    bits = forc.pack_bits(allowed)
    assert bits.shape == (3, 3) and bits.dtype == np.uint32
    assert np.array_equal(forc.unpack_bits(bits, 77), allowed)
    assert bits[0, 0] & 1 == allowed[0, 0] and (bits[1, 2] >> 12) & 1 == allowed[1, 76]     # slot 76: word 2, bit 12
    adr = np.array([5, -1, 76, 77, 10 ** 12, 5, 31, 32], np.int64)      # -1, the capacity and beyond are ignored
    row = forc.build_bits(adr, 77, stride=5)
    assert list(np.flatnonzero(forc.unpack_bits(row, 77)[0])) == [5, 31, 32, 76] and not row[3:].any()


def test_oracle_filter_rules():
    """a row is a set of extra tombstones; a row outside [0, n_filters) allows nothing; NaN never enters; the order is
    (value descending, address ascending) and the pads are (-inf, -1)"""
    rng = np.random.default_rng(1)
    m, cap = 4, 70
    storage = rng.integers(0, 256, (1, cap, 4), dtype=np.uint8)
    storage[0, 40:50] = storage[0, 12]                                     # eleven equal codes
    lut = rng.standard_normal((m, 4, 256)).astype(np.float32)
    lut[1, 3] = np.nan                                                     # query 3: every value is NaN
    start, size = np.array([[0, 32]] * 4, np.int64), np.array([[32, 60]] * 4, np.int64)   # the second cell is cut at 70
    npl = np.full(4, 2, np.int64)
    is_empty = np.zeros(cap, np.uint8)
    is_empty[[3, 45]] = 1
    allowed = np.zeros((2, cap), bool)
    allowed[0] = True
    allowed[1, [3, 12, 41, 45, 47, 69]] = True
    rows = np.array([0, 1, 2, 0], np.int32)
    v, a = forc.scan_filtered(storage, lut, is_empty, allowed, rows, start, size, npl, 8)
    ev, ea = orc.scan_topk(storage, lut, is_empty, np.minimum(start, cap), np.minimum(size, cap - start), npl, 8)
    assert np.array_equal(a[0], ea[0]) and np.array_equal(v[0].view(np.uint32), ev[0].view(np.uint32))
    assert list(a[1][4:]) == [-1] * 4 and sorted(a[1][:4]) == [12, 41, 47, 69] and np.all(np.isneginf(v[1][4:]))
    assert list(a[1][:4]) == list(a[1][:4][np.lexsort((a[1][:4], -v[1][:4].astype(np.float64)))])
    tied = [i for i in range(4) if a[1][i] in (12, 41, 47)]
    assert [a[1][i] for i in tied] == [12, 41, 47] and len({v[1][i] for i in tied}) == 1    # equal values: by address
    assert np.all(a[2] == -1) and np.all(a[3] == -1)                       # no such row; every value NaN
    v0, a0 = forc.scan_filtered(storage, lut, is_empty, allowed, None, start, size, npl, 8)   # no rows given: row 0
    assert np.array_equal(a0[0], a[0]) and (a0[1] >= 0).all() and not np.array_equal(a0[1], a[1])


@pytest.mark.parametrize("k", [1, 10, 100, 1000])
def test_all_ones_row_equals_the_topk_oracle(k):
    """with the all-ones row on a layout whose cells stay inside the storage the filtered oracle is orc.scan_topk"""
    case = cases.plain_case(16, 4, "fused", 3, 8, "euclidean", over=False)
    ev, ea = orc.scan_topk(case["storage"], case["lut"], case["is_empty"], case["cs"], case["sz"], case["npl"], k)
    for rows in (None, np.zeros(3, np.int32)):
        v, a = forc.scan_filtered(case["storage"], case["lut"], case["is_empty"], case["allowed"], rows, case["cs"],
                                  case["sz"], case["npl"], k)
        assert np.array_equal(a, ea) and np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    res = cases.residual_case(8, 4, "part1", 3, 8, over=False)
    ev, ea = orc.scan_topk_residual(res["storage"], res["part1"], res["part2"], res["cells"], res["base_sims"],
                                    res["is_empty"], res["cs"], res["sz"], res["npl"], k)
    v, a = forc.scan_filtered_residual(res["storage"], res["part1"], res["part2"], res["cells"], res["base_sims"],
                                       res["is_empty"], res["allowed"], None, res["cs"], res["sz"], res["npl"], k)
    assert np.array_equal(a, ea) and np.array_equal(v.view(np.uint32), ev.view(np.uint32))


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------
def _case_is_what_the_gpu_tests_claim(case, nq, n_probe):
    cap = case["storage"].shape[1]
    assert cap % 32 != 0                                                 # the last filter word is partly padding
    assert all(cases.conditions(case).values()), cases.conditions(case)
    allowed, live = case["allowed"], case["is_empty"] == 0
    assert allowed.shape == (len(cases.ROWS), cap)
    assert allowed[0].all() and not (allowed[1] & live).any()            # all ones; all zeros on the live slots
    start = case["big_start"]
    big = np.zeros(cap, bool)
    big[start:start + 300] = True
    assert (allowed[2] & live).sum() == 1 and (allowed[2] & live & big).sum() == 1
    assert 0.01 < (allowed[3] & live).sum() / live.sum() < 0.06 and 0.4 < (allowed[4] & live).sum() / live.sum() < 0.6
    # every row has bits on the tombstones, on the free slots and in the padding; none of them is a result
    assert (allowed[:, ~live]).all() and (~live).sum() > 25
    bits = case["bits"]
    assert bits.shape == (len(cases.ROWS), (cap + 31) // 32 + cases.PAD_WORDS)
    assert np.array_equal(forc.unpack_bits(bits, cap), allowed)
    assert (bits[:, -cases.PAD_WORDS:] == 0xFFFFFFFF).all() and (bits[:, cap >> 5] >> (cap & 31)).all()
    for (r, k), (v, a) in case["want"].items():
        got = a[a >= 0]
        assert live[got].all() and got.max(initial=0) < cap
        rows = case["runs"][r]
        for q in range(nq):
            row = 0 if rows is None else rows[q]
            assert allowed[row][a[q][a[q] >= 0]].all()
    over = (case["cs"] + case["sz"] > cap)
    assert over[0].any()                                                 # query 0 probes the cell that leaves the storage
    if nq > 1 and n_probe > 1:
        assert case["cs"][1, 1] == case["cs"][1, 0]                      # one cell listed twice in a row
    if nq >= 3:
        assert case["npl"][-1] == 0 and all(len(c[-1][0]) == 0 for c in case["cand"])
    if nq >= 100:
        assert (case["npl"] > n_probe).any() and (case["npl"] < n_probe).any() and (case["npl"] == n_probe).any()
    assert case["runs"][-1] is None and len(case["runs"]) == (len(cases.ROWS) + 1 if nq <= 3 else 2)
    assert {int(r) for rows in case["runs"][:-1] for r in rows} == set(range(len(cases.ROWS)))   # every row is used


@pytest.mark.parametrize("m,ds,table,nq,n_probe,metric", cases.PLAIN_CASES)
def test_gpu_plain_cases_are_not_vacuous(m, ds, table, nq, n_probe, metric):
    case = cases.plain_case(m, ds, table, nq, n_probe, metric)
    _case_is_what_the_gpu_tests_claim(case, nq, n_probe)
    assert case["lut"].shape == (m, nq, 256) and np.isfinite(case["lut"]).all()
    assert m <= cases.MAX_M and max(c[0] for c in cases.PLAIN_CASES) == cases.MAX_M


@pytest.mark.parametrize("m,ds,tables,nq,n_probe", cases.RESIDUAL_CASES)
def test_gpu_residual_cases_are_not_vacuous(m, ds, tables, nq, n_probe):
    case = cases.residual_case(m, ds, tables, nq, n_probe)
    _case_is_what_the_gpu_tests_claim(case, nq, n_probe)
    assert (case["full"] is not None) == (tables == "full")
