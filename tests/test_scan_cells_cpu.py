"""CPU: the cell-major form of the m = 64 large-batch scan route (csrc/scan_cells.hip) as far as it shows without a GPU
-- the entry points are declared, exported and bound; null pointers are rejected before any HIP call; the host rule
takes the headline call and declines the 100 M-slot call, k = 129, residual PQ, a caller's table, n_probe <= P0 and a
workspace one byte short; the workspace size itself is what it was."""
import os
import re

from conftest import ROOT

P0 = 4  # kCellP0 (csrc/scan_cells.h)


def _lib():
    from torchpq_amd import _lib
    return _lib, _lib.load()


def test_entry_points_are_declared_exported_and_bound():
    _lib_mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    build_sh = open(os.path.join(ROOT, "torchpq_amd", "csrc", "build.sh")).read()
    assert "scan_cells.hip" in build_sh
    for name in ("tpq_ivfpq_search_fused_cells", "tpq_ivfpq_scan_cell_major", "tpq_ivfpq_cell_candidates",
                 "tpq_ivfpq_cell_candidates_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib_mod.SIGNATURES and hasattr(lib, name), name
    from torchpq_amd import kernels as K
    scan = K.IVFPQTopkHip(m=64)
    assert callable(K.CellCandidatesHip) and hasattr(scan, "last_cell_major") and scan.last_cell_major() is None
    src = open(os.path.join(ROOT, "torchpq_amd", "csrc", "scan_cells.h")).read()
    assert re.search(r"define TPQ_CELL_P0 %d\b" % P0, src)


def test_null_pointers_are_rejected_before_any_hip_call():
    _lib_mod, lib = _lib()
    rc = lib.tpq_ivfpq_cell_candidates(None, None, None, 2, 0, None, None, None, None, None, 8, 0, None, 1000, 10, 8, 64,
                                       1024, None, None, None, None, None, None, 0, None)
    assert rc == -1 and "null pointer" in _lib_mod.last_error()
    rc = lib.tpq_ivfpq_search_fused_cells(None, None, None, None, 2, 0, None, None, None, None, None, None, None, None,
                                          1000, 10, 8, 64, 10, 1, None, 0, None, 0, None, 8, None)
    assert rc == -1 and "null pointer" in _lib_mod.last_error()


def _cell_major(lib, nq=10000, k=100, m=64, ds=2, n_probe=32, hint=31264, has_lut=0, residual=0, n_cells=1024,
                n_slots=1000448, ws=None):
    if ws is None:
        ws = lib.tpq_ivfpq_scan_workspace_bytes(nq, k, 1, m)
    return lib.tpq_ivfpq_scan_cell_major(nq, k, 1, m, ds, n_probe, hint, has_lut, 1, 0, residual, n_cells, n_slots, ws)


def test_rule_takes_the_headline_and_declines_the_rest():
    _lib_mod, lib = _lib()
    assert lib.tpq_ivfpq_scan_route(10000, 100, 1, 64, 2, 32, 31264, 0, 1, 0, 0) == 16      # the route stays what it was
    assert _cell_major(lib) == 1                                                            # the headline call
    # the 100 M-slot workload: 16 384 cells, 64 probes, ~39 queries per cell
    assert _cell_major(lib, n_probe=64, hint=64 * 6104, n_cells=16384, n_slots=16384 * 6104) == 0
    assert _cell_major(lib, k=128) == 1 and _cell_major(lib, k=129) == 0
    assert _cell_major(lib, residual=1) == 0
    assert _cell_major(lib, has_lut=1) == 0                                                 # a caller's table
    small = dict(n_cells=128, n_slots=128 * 977)                                            # (dense at few probes)
    assert _cell_major(lib, n_probe=P0 + 1, hint=(P0 + 1) * 977, **small) == 1
    assert _cell_major(lib, n_probe=P0, hint=P0 * 977, **small) == 0
    assert _cell_major(lib, n_probe=P0 + 1, hint=(P0 + 1) * 977) == 0                       # 49 queries per cell: sparse
    assert _cell_major(lib, nq=1000, n_cells=8, n_slots=8000, hint=8000) == 0               # below the large-batch route
    assert _cell_major(lib, m=32, ds=4) == 0 and _cell_major(lib, ds=4) == 0
    assert _cell_major(lib, nq=0) == -1                                                     # rejected like the route query


def _extras(nq, n_probe, n_cells):
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    return (256 + 4 * align(nq * 4) + align(n_cells * 4) + 2 * align((n_cells + 1) * 4) + 2 * align(n_cells * 4)
            + align(nq * (n_probe - P0) * 4) + align(nq * 512))


def test_form_needs_room_behind_the_lists_in_use():
    """the form keeps a query's lists as 16 chunks of 64 keys (8 when 16 do not fit: k <= 56, whose workspace is that
    of 16 chunks alone) and its inversion arrays behind them"""
    _lib_mod, lib = _lib()
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    nq = 10000
    lists = lambda chunks: 2 * align(nq * 4) + nq * chunks * 64 * 8 + align(nq * chunks * 4)  # noqa: E731
    need8 = lists(8) + _extras(nq, 32, 1024)
    assert _cell_major(lib, ws=need8) == 1 and _cell_major(lib, ws=need8 - 1) == 0 and _cell_major(lib, ws=0) == 0
    assert lists(16) + _extras(nq, 32, 1024) < lib.tpq_ivfpq_scan_workspace_bytes(nq, 100, 1, 64)
    assert need8 < lib.tpq_ivfpq_scan_workspace_bytes(nq, 10, 1, 64) < lists(16) + _extras(nq, 32, 1024)
    assert _cell_major(lib, k=10) == 1


def test_workspace_size_is_unchanged():
    _lib_mod, lib = _lib()
    assert lib.tpq_ivfpq_scan_workspace_bytes(100, 100, 1, 64) == 2 * 512 + 100 * 16 * 128 * 8 + 6400
    assert lib.tpq_ivfpq_scan_workspace_bytes(10000, 100, 1, 64) == 2 * 40192 + 10000 * 16 * 128 * 8 + 640000
    assert lib.tpq_ivfpq_scan_workspace_bytes(10000, 10, 1, 64) == 2 * 40192 + 10000 * 16 * 64 * 8 + 640000
    assert lib.tpq_ivfpq_cell_candidates_workspace_bytes(10000, 32, 1024, P0) == _extras(10000, 32, 1024)
