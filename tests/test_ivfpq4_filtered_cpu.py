"""CPU: the surface of IVFPQ4Index filtered search -- the two C-ABI symbols and their validation, the wrapper and the
index methods --, the filtered oracle (tests/ivfpq4_filtered_oracle.py) against the unfiltered oracles where they must
agree, and the conditions on the inputs of the GPU tests (tests/ivfpq4_filtered_cases.py), asserted on the oracle
alone."""
import ctypes as C
import inspect
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

import ivfpq4_filtered_cases as cases
import ivfpq4_filtered_guarded as guarded
import ivfpq4_filtered_oracle as forc
import ivfpq4_oracle as porc
import ivfpq4_residual_cases as rcases
import ivfpq_filtered_cases as fcases
from conftest import ROOT

PLAIN, RESIDUAL = "tpq_ivfpq4_scan_filtered_topk", "tpq_ivfpq4_scan_filtered_residual_topk"


def test_symbols_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    lib = _lib.load()
    for name in (PLAIN, RESIDUAL):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    res, args = _lib.SIGNATURES[PLAIN]
    assert res is C.c_int and len(args) == 24 and args[9] is C.c_int and args[10] is C.c_int64
    assert args[13] is C.c_int64 and args[22] is C.c_size_t
    res, args = _lib.SIGNATURES[RESIDUAL]
    assert res is C.c_int and len(args) == 27 and args[5] is C.c_int and args[12] is C.c_int and args[13] is C.c_int64
    assert args[16] is C.c_int64 and args[25] is C.c_size_t
    # the workspace is the unfiltered scan's: no sizing symbol of its own
    assert not [s for s in _lib.SIGNATURES if "ivfpq4" in s and "filtered" in s and "workspace" in s]


def _entry_points():
    """(name, all-NULL arguments with a valid shape, the position of n_filters -- filter_stride follows it --, the
    position of n_slots -- m, ds, nq, max_nprobe, k, metric and n_split follow it)"""
    N_ = None
    #        codes query codebook empty start size npl bits ofq nf stride vals addr n_slots m ds nq np k metric split
    plain = [N_, N_, N_, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, 100, 8, 2, 1, 4, 10, 0, 1, N_, 0, N_]
    #      codes query codebook centroids cells n_cells empty start size npl bits ofq nf stride vals addr n_slots ...
    res = [N_, N_, N_, N_, N_, 3, N_, N_, N_, N_, N_, N_, 1, 4, N_, N_, 100, 8, 2, 1, 4, 10, 0, 1, N_, 0, N_]
    return ((PLAIN, plain, 9, 13), (RESIDUAL, res, 12, 16))


def test_arguments_are_checked_before_any_hip_call():
    """no GPU here: every rejection below happens before the library touches HIP"""
    from torchpq_amd import _lib
    lib = _lib.load()
    room = (C.c_char * 64)()                          # a non-NULL pointer nothing dereferences
    for name, args, nf, n0 in _entry_points():
        fn = getattr(lib, name)
        M, DS, NQ, NP, K, METRIC, SPLIT = (n0 + i for i in range(1, 8))

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
        for k in (0, 1025):
            assert at(K, k) == _lib.ERR_UNSUPPORTED and "k=%d" % k in _lib.last_error(), (name, k)
        for n_split in (0, 1025):
            assert at(SPLIT, n_split) == -1 and "n_split" in _lib.last_error(), (name, n_split)
        assert at(METRIC, 7) == -1 and "metric" in _lib.last_error()
        assert at(NP, 0) == -1 and at(NQ, -1) == -1 and at(n0, -1) == -1
        for n_filters in (0, -2):
            assert at(nf, n_filters) == -1 and "n_filters" in _lib.last_error(), (name, n_filters)
        assert at(nf + 1, 3) == -1 and "filter_stride" in _lib.last_error()      # one word short of ceil(100 / 32)
        assert call(**{"p%d" % n0: (1 << 31) - 1, "p%d" % (nf + 1): 1 << 26}) == _lib.ERR_UNSUPPORTED
        assert "2^31" in _lib.last_error()
        assert at(NQ, 0) == 0                          # no queries: nothing to do
        # every pointer given but the filter's bits
        full = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
        a = list(full)
        a[nf - 2] = None
        assert fn(*a) == -1 and "null pointer" in _lib.last_error(), name
        a = list(full)
        a[nf - 1] = None                               # no filter_of_query is row 0, not an error: the next check
        a[SPLIT], a[SPLIT + 1], a[SPLIT + 2] = 2, None, 0                         # ... a split scan needs a workspace
        assert fn(*a) == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error(), name
        # m = 256 with sub-vectors of 160 floats: the staged query alone is 160 KiB
        a = list(full)
        a[M], a[DS] = 256, 160
        assert fn(*a) == _lib.ERR_UNSUPPORTED and "LDS" in _lib.last_error(), name
    name, args, nf, n0 = _entry_points()[1]
    a = list(args)
    a[5] = 0
    assert getattr(lib, name)(*a) == -1 and "n_cells" in _lib.last_error()
    full = [C.addressof(room) if v is None else v for v in args[:-1]] + [None]
    for pos in (3, 4):                                 # centroids, cells
        a = list(full)
        a[pos] = None
        assert getattr(lib, name)(*a) == -1 and "null pointer" in _lib.last_error()


def test_wrapper_and_index_methods_exist():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    empty = inspect.Parameter.empty
    params = lambda fn: [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
    assert "IVFPQ4FilteredTopkHip" in kernels.__all__ and callable(kernels.IVFPQ4FilteredTopkHip)
    op = kernels.IVFPQ4FilteredTopkHip(m=8)
    assert op.last_n_split is None and callable(op.residual)
    assert kernels.IVFPQ4FilteredTopkHip._n_split is kernels.IVFPQ4TopkHip._n_split
    for bad in (4, 12, 264):
        with pytest.raises(AssertionError):
            kernels.IVFPQ4FilteredTopkHip(m=bad)
    assert [n for n, _ in params(op.__call__.__func__)] == [
        n for n, _ in params(kernels.IVFPQ4TopkHip.__call__)][:7] + [
        "filter_bits", "filter_of_query", "is_empty", "distance", "n_split", "slots_hint"]
    assert [n for n, _ in params(op.residual.__func__)] == [
        n for n, _ in params(kernels.IVFPQ4ResidualTopkHip.__call__)][:9] + [
        "filter_bits", "filter_of_query", "is_empty", "distance", "n_split", "slots_hint"]
    for method in ("search_filtered", "search_cells_filtered", "id_filter"):
        assert params(getattr(index.IVFPQ4Index, method)) == params(getattr(index.IVFPQIndex, method)), method
    assert params(index.IVFPQ4Index.search_filtered) == [
        ("x", empty), ("k", empty), ("flt", empty), ("filter_of_query", None)]
    assert "search_filtered" in sys.modules[index.IVFPQ4Index.__module__].__doc__
    assert "IVFPQ4Index" in sys.modules["torchpq_amd.index._filter"].__doc__


def test_wrapper_declines_cpu_tensors_and_bad_filters():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFPQ4FilteredTopkHip
    op = IVFPQ4FilteredTopkHip(m=8)
    codes, query, codebook = torch.zeros(1, 100, 4, dtype=torch.uint8), torch.zeros(16, 2), torch.zeros(8, 2, 16)
    cs, sz, npl = torch.zeros(2, 1, dtype=torch.long), torch.full((2, 1), 10), torch.ones(2, dtype=torch.long)
    centroids = torch.zeros(3, 16)
    bits, rows = torch.zeros(1, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    plain = lambda *a, **kw: op(codes, query, codebook, cs, sz, npl, *a, **kw)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        plain(5, bits, rows)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        op.residual(codes, query, codebook, centroids, cs, cs, sz, npl, 5, bits)
    with pytest.raises(AssertionError):
        plain(5, bits[:, :3])                                              # a row one word short of the storage
    with pytest.raises(AssertionError):
        plain(5, bits.long())
    with pytest.raises(AssertionError):
        plain(5, bits, rows.long())                                        # int32 at the C ABI
    with pytest.raises(AssertionError):
        plain(5, bits, rows[:1])                                           # one row per query
    with pytest.raises(AssertionError):
        plain(1025, bits)
    with pytest.raises(AssertionError):
        op.residual(codes, query, codebook, centroids[:, :-1], cs, cs, sz, npl, 5, bits)   # another d
    with pytest.raises(AssertionError):
        op.residual(codes, query, codebook, centroids, cs[:1], cs, sz, npl, 5, bits)       # cells of another batch


class _Stub:
    """what search_filtered, search_cells_filtered and IdFilter ask of an index before any kernel runs"""
    device = "cpu"
    n_probe, n_cells, capacity, _codes_version = 1, 4, 64, 0
    vq_codec = pq_codec = types.SimpleNamespace(is_trained=True)

    def _prepare(self, x):
        return x

    def _search_batches(self, x, per_batch, alongside=()):
        raise RuntimeError("the checks passed")

    def _scan_preamble(self, x, cells, n_probe_list, extents):
        return n_probe_list, None, None, 0, None


def test_index_rejects_foreign_filters_and_bad_rows():
    from torchpq_amd.index import IVFPQ4Index
    from torchpq_amd.index._filter import IdFilter
    me, other = _Stub(), _Stub()
    x = torch.zeros(8, 3)
    mine = IdFilter(me, torch.arange(5))
    search = lambda *a: IVFPQ4Index.search_filtered(me, x, 5, *a)
    with pytest.raises(RuntimeError, match="the checks passed"):
        search(mine, torch.zeros(3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="the checks passed"):
        search(mine, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(AssertionError):
        search(mine, torch.zeros(2, dtype=torch.int32))                    # one row per query
    with pytest.raises(AssertionError):
        search(mine, torch.zeros(3, 1, dtype=torch.int32))
    with pytest.raises(AssertionError):
        search(mine, torch.zeros(3))                                       # a float tensor
    with pytest.raises(AssertionError):
        search(mine, [0, 0, 0])
    with pytest.raises(AssertionError, match="id_filter"):
        search(torch.arange(5))                                            # ids, not a filter
    with pytest.raises(AssertionError):
        IVFPQ4Index.search_filtered(me, x, 0, mine)
    with pytest.raises(AssertionError):
        IVFPQ4Index.search_filtered(me, x, 1025, mine)
    cells = torch.zeros(3, 1, dtype=torch.long)
    with pytest.raises(AssertionError, match="another index"):
        IVFPQ4Index.search_cells_filtered(me, x, cells, IdFilter(other, torch.arange(5)))
    assert isinstance(IVFPQ4Index.id_filter(me, torch.arange(5)), IdFilter)


# ---- the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("k", [1, 10, 100, 1024])
def test_all_ones_row_equals_the_unfiltered_oracle(k, residual):
    c = cases.case(24, 2, 3, 4, "euclidean", residual)
    if residual:
        ev, ea = rcases.scan(c, k, "euclidean")
    else:
        ev, ea = porc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"], c["cs"], c["sz"], c["npl"], k)
    assert c["runs"][-1] is None
    for got in (cases.want(c, len(c["runs"]) - 1, k),
                forc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"], c["allowed"],
                               np.zeros(3, np.int32), c["cs"], c["sz"], c["npl"], k, "euclidean",
                               **(dict(centroids=c["centroids"], cells=c["cells"]) if residual else {}))):
        assert np.array_equal(got[1], ea) and np.array_equal(got[0].view(np.uint32), ev.view(np.uint32))
    assert (ea >= 0).any()


def test_oracle_filter_rules():
    """a row is a set of extra tombstones; a row outside [0, n_filters) allows nothing; the pads are (-inf, -1)"""
    c = cases.case(8, 2, 3, 8, "inner", False)
    rows = np.array([4, -1, len(cases.ROWS)], np.int32)
    v, a = forc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"], c["allowed"], rows, c["cs"],
                          c["sz"], c["npl"], 50, "inner")
    assert np.all(a[1:] == -1) and np.all(np.isneginf(v[1:]))
    got = a[0][a[0] >= 0]
    assert len(got) and c["allowed"][4][got].all() and (c["is_empty"][got] == 0).all()
    assert np.all(v[0][:-1] >= v[0][1:])
    mask = forc.row_mask(c["is_empty"], c["allowed"], 4)
    ev, ea = porc.scan_topk(c["storage"], c["query"], c["codebook"], mask, c["cs"], c["sz"], c["npl"], 50, "inner")
    assert np.array_equal(a[0], ea[0]) and np.array_equal(v[0].view(np.uint32), ev[0].view(np.uint32))
    assert forc.row_mask(None, c["allowed"], 0).sum() == 0 and forc.row_mask(None, c["allowed"], 9).all()


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("m,ds,nq,n_probe,distance", cases.KERNEL_CASES)
def test_gpu_cases_are_not_vacuous(m, ds, nq, n_probe, distance, residual):
    c = cases.case(m, ds, nq, n_probe, distance, residual)
    cap = c["storage"].shape[1]
    assert cap % 32 != 0                                                 # the last filter word is partly padding
    cond = fcases.conditions(c)
    assert set(cond) == {"fewer", "differs", "tie", "empty_tile", "sparse_seen"} and all(cond.values()), cond
    allowed, live = c["allowed"], c["is_empty"] == 0
    assert allowed.shape == (len(cases.ROWS), cap)
    assert allowed[0].all() and not (allowed[1] & live).any()            # all ones; all zeros on the live slots
    start = c["big_start"]
    assert (allowed[2] & live).sum() == 1 and start <= np.flatnonzero(allowed[2] & live)[0] < start + 300
    assert not (allowed[3] & live)[start + 64:start + 128].any() and (allowed[3] & live)[start:start + 64].any()
    assert 0.4 < (allowed[4] & live).sum() / live.sum() < 0.6
    # every row has bits on the tombstones, on the free slots and in the padding; none of them is a result
    assert allowed[:, ~live].all() and (~live).sum() > 25
    bits = c["bits"]
    assert bits.shape == (len(cases.ROWS), (cap + 31) // 32 + fcases.PAD_WORDS)
    assert np.array_equal(forc.unpack_bits(bits, cap), allowed)
    assert (bits[:, -fcases.PAD_WORDS:] == 0xFFFFFFFF).all() and (bits[:, cap >> 5] >> (cap & 31)).all()
    for run, rows in enumerate(c["runs"]):
        v, a = cases.want(c, run, 1024)
        assert (a >= 0).sum(1).max() < 1024                              # the full depth holds every candidate
        for q in range(nq):
            got = a[q][a[q] >= 0]
            assert live[got].all() and allowed[0 if rows is None else rows[q]][got].all()
    assert c["runs"][-1] is None and len(c["runs"]) == (len(cases.ROWS) + 1 if nq <= 3 else 2)
    assert {int(r) for rows in c["runs"][:-1] for r in rows} == set(range(len(cases.ROWS)))   # every row is used
    if nq > 1 and n_probe > 1:
        assert c["cs"][1, 1] == c["cs"][1, 0]                            # one cell listed twice in a row
    if m == 256 and n_probe == 8:
        assert 32 * 1024 // (m * 64) == 2                                # two tables per buffer: four groups


def test_mixed_table_case_allows_eight_to_twelve_live_slots_per_cell():
    c = cases.mixed_table_case()
    live = c["is_empty"] == 0
    seen = set()
    for start, size in zip(c["cs"].ravel(), c["sz"].ravel()):
        n_live = int(live[start:start + size].sum())
        n = int((c["allowed"][0] & live)[start:start + size].sum())
        assert (8 <= n <= 12) if n_live >= 12 else n == n_live, (start, size, n)
        seen.add(int(size))
    assert seen == set(rcases.CELL_SIZES)                                # every cell is probed by some query
    assert len(np.unique(c["storage"].reshape(c["storage"].shape[0], -1, 4), axis=1)[0]) == 1   # one code everywhere
    # row 1: tiles 0 and 4 of the 300-slot cell, and nothing else
    start = c["big_start"]
    only = c["allowed"][1] & live
    assert only[start:start + 64].any() and only[start + 256:start + 300].any()
    assert not only[start + 64:start + 256].any() and only.sum() == only[start:start + 300].sum()
    assert np.array_equal(forc.unpack_bits(c["bits"], len(live)), c["allowed"])


def test_both_entry_points_have_a_guarded_case():
    """the table of tests/guarded_cases.py holds a case for each new entry point, with a builder in
    tests/test_gpu_guarded_buffers.BUILDERS (registered by tests/ivfpq4_filtered_guarded.py)"""
    import guarded_cases
    import test_gpu_guarded_buffers as gpu
    for cid, symbols in guarded.CASE_SYMBOLS.items():
        assert guarded_cases.CASE_SYMBOLS[cid] == symbols and guarded_cases.CASE_IDS.count(cid) == 1
        assert callable(gpu.BUILDERS[cid]) and cid not in guarded_cases.NOT_BIT_EXACT
        for s in symbols:
            assert guarded_cases.CASES[s] == [cid]
    assert {PLAIN, RESIDUAL} == {s for symbols in guarded.CASE_SYMBOLS.values() for s in symbols}
    guarded.register()                                                   # (a second registration changes nothing)
    assert len(guarded_cases.CASE_IDS) == len(set(guarded_cases.CASE_IDS)) == len(gpu.BUILDERS)
