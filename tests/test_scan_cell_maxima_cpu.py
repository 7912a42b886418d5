"""CPU: the threshold form of the cell-major scan (csrc/scan_cells.hip, `The threshold from group maxima`) as far as it
shows without a GPU -- the entry points are declared, exported and bound; the host rule takes the headline call and
declines n_probe <= T, a workspace of exactly lists + extras + norms, k = 129, residual PQ, a caller's table and the short
cells of the seeded form's tests; the switch returns the previous setting; the workspace sizes
are what they were; and a numpy model of the bound in the kernel's
row-to-lane grouping: the k-th largest group maximum never exceeds the k-th largest value, whatever subset of the maxima
is dropped."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

P0 = 4


def _constants():
    src = open(os.path.join(ROOT, "torchpq_amd", "csrc", "scan_cells.h")).read()
    t = int(re.search(r"define TPQ_CELL_THR_PROBES (\d+)", src).group(1))
    g = int(re.search(r"define TPQ_CELL_THR_GROUP (\d+)", src).group(1))
    return t, g


T, G = _constants()


def _lib():
    from torchpq_amd import _lib
    return _lib, _lib.load()


def _ask(lib, name, nq=10000, k=100, m=64, ds=2, n_probe=32, hint=31264, has_lut=0, residual=0, n_cells=1024,
         n_slots=1000448, ws=None):
    if ws is None:
        ws = lib.tpq_ivfpq_scan_workspace_bytes(nq, k, 1, m)
    return getattr(lib, name)(nq, k, 1, m, ds, n_probe, hint, has_lut, 1, 0, residual, n_cells, n_slots, ws)


def _thr(lib, **kw):
    return _ask(lib, "tpq_ivfpq_scan_cell_threshold", **kw)


def _align(n):
    return (n + 255) // 256 * 256


def _extras(nq, n_probe, n_cells):
    return (256 + 4 * _align(nq * 4) + _align(n_cells * 4) + 2 * _align((n_cells + 1) * 4) + 2 * _align(n_cells * 4)
            + _align(nq * (n_probe - P0) * 4) + _align(nq * 512))


def _thr_arrays(nq, n_probe, n_cells):
    return (_align(nq * n_probe * 4) + 3 * _align(n_cells * 4) + 2 * _align((n_cells + 1) * 4)
            + _align(nq * min(T, n_probe) * 4) + _align(nq * 4))


def test_entry_points_are_declared_exported_and_bound():
    _lib_mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in ("tpq_ivfpq_scan_cell_threshold", "tpq_ivfpq_scan_use_cell_threshold", "tpq_ivfpq_scan_cell_threshold_probes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib_mod.SIGNATURES and hasattr(lib, name), name
    from torchpq_amd import kernels as K
    scan = K.IVFPQTopkHip(m=64)
    assert scan.last_cell_threshold() is None
    from torchpq_amd.index import IVFPQIndex
    assert IVFPQIndex.use_cell_threshold is True
    assert T in (4, 6, 8) and G in (8, 16)


def test_rule_takes_the_headline_and_declines_the_rest():
    _lib_mod, lib = _lib()
    assert _ask(lib, "tpq_ivfpq_scan_cell_major") == 1 and _ask(lib, "tpq_ivfpq_scan_cell_norms") == 1
    assert _thr(lib) == 1                                                   # the headline call
    assert _thr(lib, k=128) == 1 and _thr(lib, k=129) == 0
    assert _thr(lib, residual=1) == 0
    assert _thr(lib, has_lut=1) == 0                                        # a caller's table
    dense = dict(n_cells=128, n_slots=128 * 977)
    assert _thr(lib, n_probe=T + 1, hint=(T + 1) * 977, **dense) == 1
    assert _ask(lib, "tpq_ivfpq_scan_cell_major", n_probe=max(T, P0 + 1), hint=max(T, P0 + 1) * 977, **dense) == 1
    assert _thr(lib, n_probe=T, hint=T * 977, **dense) == 0                 # nothing behind the first pass
    assert _thr(lib, nq=0) == -1                                            # rejected like the route query
    # the 100 M-slot workload is not cell-dense: no cell-major form at all
    assert _thr(lib, n_probe=64, hint=64 * 6104, n_cells=16384, n_slots=16384 * 6104) == 0


def test_rule_wants_long_cells_and_twice_k_maxima():
    """the seeded form's tests run at mean cells of 50 ... 381 slots: they keep that form"""
    _lib_mod, lib = _lib()
    for mean in (50, 170, 381, 511):
        small = dict(nq=1024, n_probe=8, hint=8 * mean, n_cells=8, n_slots=8 * (mean + 5))
        assert _ask(lib, "tpq_ivfpq_scan_cell_norms", **small) == 1, mean
        assert _thr(lib, k=1, **small) == 0, mean
    if T < 8:
        long_ = dict(nq=1024, n_probe=8, hint=8 * 512, n_cells=8, n_slots=8 * 517)
        assert _thr(lib, k=1, **long_) == 1
        k_max = T * 512 // G // 2
        if k_max < 128:
            assert _thr(lib, k=k_max, **long_) == 1 and _thr(lib, k=k_max + 1, **long_) == 0


def test_form_needs_room_behind_the_norms():
    _lib_mod, lib = _lib()
    nq, n_slots = 10000, 1000448
    lists = 2 * _align(nq * 4) + nq * 16 * 64 * 8 + _align(nq * 16 * 4)
    norms = lists + _extras(nq, 32, 1024) + _align(n_slots * 4)
    assert _ask(lib, "tpq_ivfpq_scan_cell_norms", ws=norms) == 1 and _thr(lib, ws=norms) == 0
    need = norms + _thr_arrays(nq, 32, 1024)
    assert _thr(lib, ws=need) == 1 and _thr(lib, ws=need - 1) == 0 and _thr(lib, ws=0) == 0
    assert need < lib.tpq_ivfpq_scan_workspace_bytes(nq, 100, 1, 64)


def test_switch_returns_the_previous_setting_and_leaves_the_rule_alone():
    _lib_mod, lib = _lib()
    assert lib.tpq_ivfpq_scan_cell_threshold_probes() == T
    assert lib.tpq_ivfpq_scan_use_cell_threshold(0) == 1          # on by default
    try:
        assert _thr(lib) == 1                                     # the rule is host arithmetic on the arguments alone
        assert lib.tpq_ivfpq_scan_use_cell_threshold(0) == 0
    finally:
        assert lib.tpq_ivfpq_scan_use_cell_threshold(1) == 0
    assert lib.tpq_ivfpq_scan_use_cell_threshold(1) == 1


def test_workspace_sizes_are_unchanged():
    _lib_mod, lib = _lib()
    assert lib.tpq_ivfpq_scan_workspace_bytes(10000, 100, 1, 64) == 2 * 40192 + 10000 * 16 * 128 * 8 + 640000
    assert lib.tpq_ivfpq_scan_workspace_bytes(10000, 10, 1, 64) == 2 * 40192 + 10000 * 16 * 64 * 8 + 640000
    assert lib.tpq_ivfpq_cell_candidates_workspace_bytes(10000, 32, 1024, P0) == _extras(10000, 32, 1024)
    assert lib.tpq_ivfpq_cell_candidates_norms_workspace_bytes(10000, 32, 1024, P0, 1000448) == (
        _extras(10000, 32, 1024) + _align(1000448 * 4))


# ---- the bound, in the kernel's grouping ---------------------------------------------------------------------------------
def group_maxima(values, live, group):
    """The maxima pass A stores for one (cell, query): `values` [size] the tested values of the cell's rows, `live` [size]
    bool.  A tile is 32 rows; lane half h holds, in accumulator register 4 g + i, row 8 g + 4 h + i of the tile; a group is
    `group` consecutive registers of one lane.  A group without a live row stores nothing."""
    size = len(values)
    out = []
    for r0 in range(0, size, 32):
        for half in range(2):
            rows = np.array([r0 + 8 * (r // 4) + 4 * half + (r % 4) for r in range(16)])
            for g0 in range(0, 16, group):
                rr = rows[g0:g0 + group]
                rr = rr[rr < size]
                rr = rr[live[rr]]
                if len(rr):
                    out.append(values[rr].max())
    return np.array(out)


@pytest.mark.parametrize("group", [8, 16])
@pytest.mark.parametrize("size", [1, 31, 32, 33, 1000])
def test_kth_group_maximum_never_exceeds_the_kth_value(size, group):
    rng = np.random.default_rng(100 * size + group)
    for trial in range(20):
        n_cells = int(rng.integers(1, 7))
        ties = trial % 3 == 0
        vals, maxima = [], []
        for _ in range(n_cells):
            v = rng.integers(-3, 4, size).astype(np.float32) if ties else rng.standard_normal(size).astype(np.float32)
            live = rng.random(size) >= 0.05
            vals.append(v[live])
            maxima.append(group_maxima(v, live, group))
        vals, maxima = np.sort(np.concatenate(vals))[::-1], np.concatenate(maxima)
        # every row is in exactly one group: the groups with a live row cover the live rows
        assert len(maxima) <= len(vals) and (len(vals) == 0 or maxima.max() == vals[0])
        for drop in (0.0, 0.3, 0.9):
            kept = np.sort(maxima[rng.random(len(maxima)) >= drop])[::-1]
            for k in (1, 2, 10, 100, 128):
                if len(kept) >= k:       # (fewer than k maxima: the threshold is -inf)
                    assert kept[k - 1] <= vals[k - 1], (size, group, drop, k)
