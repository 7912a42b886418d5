"""CPU: the per-call slot norms of the cell-major form (cell_norm_kernel, csrc/scan_cells.hip) as far as they show without
a GPU -- the host query tpq_ivfpq_scan_cell_norms says which candidate kernel a call takes: the one that reads the norms
of an array computed once per call when the workspace has room for it behind the lists and inversion arrays in use, the
one that forms them in every block otherwise; and the size function of the candidate pass with that room."""
import os
import re

from conftest import ROOT

P0 = 4  # kCellP0 (csrc/scan_cells.h)
HEADLINE = dict(nq=10000, k=100, m=64, ds=2, n_probe=32, hint=31264, has_lut=0, residual=0, n_cells=1024, n_slots=1000448)


def _lib():
    from torchpq_amd import _lib
    return _lib, _lib.load()


def _align(n):
    return (n + 255) // 256 * 256


def _extras(nq, n_probe, n_cells, p0=P0):
    return (256 + 4 * _align(nq * 4) + _align(n_cells * 4) + 2 * _align((n_cells + 1) * 4) + 2 * _align(n_cells * 4)
            + _align(nq * (n_probe - p0) * 4) + _align(nq * 512))


def _lists(nq, chunks):
    return 2 * _align(nq * 4) + nq * chunks * 64 * 8 + _align(nq * chunks * 4)


def _ask(lib, name, ws=None, **kw):
    a = dict(HEADLINE, **kw)
    if ws is None:
        ws = lib.tpq_ivfpq_scan_workspace_bytes(a["nq"], a["k"], 1, a["m"])
    return getattr(lib, name)(a["nq"], a["k"], 1, a["m"], a["ds"], a["n_probe"], a["hint"], a["has_lut"], 1, 0,
                              a["residual"], a["n_cells"], a["n_slots"], ws)


def _norms(lib, **kw):
    return _ask(lib, "tpq_ivfpq_scan_cell_norms", **kw)


def _form(lib, **kw):
    return _ask(lib, "tpq_ivfpq_scan_cell_major", **kw)


def test_entry_points_are_declared_exported_and_bound():
    _lib_mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in ("tpq_ivfpq_scan_cell_norms", "tpq_ivfpq_cell_candidates_norms_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib_mod.SIGNATURES and hasattr(lib, name), name
    from torchpq_amd import kernels as K
    scan = K.IVFPQTopkHip(m=64)
    assert hasattr(scan, "last_cell_norms") and scan.last_cell_norms() is None


def test_headline_call_takes_the_norms_with_the_librarys_own_workspace():
    _lib_mod, lib = _lib()
    assert _form(lib) == 1 and _norms(lib) == 1
    assert _norms(lib, k=10) == 1          # (8 chunks: the norms still fit the workspace of 16 lists of 64 keys)


def test_no_room_behind_the_extras_keeps_the_chain():
    _lib_mod, lib = _lib()
    nq, n_slots = HEADLINE["nq"], HEADLINE["n_slots"]
    extras = _extras(nq, 32, 1024)
    for chunks in (16, 8):
        exact = _lists(nq, chunks) + extras
        assert _form(lib, ws=exact) == 1 and _norms(lib, ws=exact) == 0
    # the boundary: the norms are align256(4 n_slots) bytes behind the lists in use and the extras
    room = _lists(nq, 16) + extras + _align(4 * n_slots)
    assert _norms(lib, ws=room) == 1 and _norms(lib, ws=room - 1) == 0
    # between the two list forms the call keeps 8 chunks; the norms need their room behind those
    room8 = _lists(nq, 8) + extras + _align(4 * n_slots)
    assert room8 < _lists(nq, 16) + extras
    assert _norms(lib, ws=room8) == 1 and _norms(lib, ws=room8 - 1) == 0 and _form(lib, ws=room8 - 1) == 1


def test_zero_wherever_the_form_is_declined():
    _lib_mod, lib = _lib()
    small = dict(n_cells=128, n_slots=128 * 977)
    declined = [dict(n_probe=64, hint=64 * 6104, n_cells=16384, n_slots=16384 * 6104), dict(k=129), dict(residual=1),
                dict(has_lut=1), dict(n_probe=P0, hint=P0 * 977, **small), dict(n_probe=P0 + 1, hint=(P0 + 1) * 977),
                dict(nq=1000, n_cells=8, n_slots=8000, hint=8000), dict(m=32, ds=4), dict(ds=4), dict(ws=0)]
    for kw in declined:
        assert _form(lib, **kw) == 0 and _norms(lib, **kw) == 0, kw
    assert _norms(lib, nq=0) == -1 and _form(lib, nq=0) == -1
    taken = [dict(), dict(k=128), dict(n_probe=P0 + 1, hint=(P0 + 1) * 977, **small)]
    for kw in taken:
        assert _form(lib, **kw) == 1 and _norms(lib, **kw) == 1, kw


def test_size_function_is_extras_plus_the_norms():
    _lib_mod, lib = _lib()
    f = lib.tpq_ivfpq_cell_candidates_norms_workspace_bytes
    for nq, n_probe, n_cells, p0, n_slots in ((10000, 32, 1024, P0, 1000448), (96, 7, 7, 1, 248), (1, 1, 1, 0, 0),
                                               (300, 6, 8, 2, 63)):
        assert lib.tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, n_cells, p0) == _extras(nq, n_probe, n_cells, p0)
        assert f(nq, n_probe, n_cells, p0, n_slots) == _extras(nq, n_probe, n_cells, p0) + _align(4 * n_slots)
    assert f(0, 32, 1024, P0, 1000) == 0 and f(10, 32, 1024, P0, -1) == 0
