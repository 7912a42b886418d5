"""CPU: the dispatch order of the large-batch scan routes (csrc/scan_order.hip) as far as it shows without a GPU -- the
entry points are declared, exported and bound; the plan orders a batch exactly when it needs more than one round of the
given workgroup slots, rides a large-batch route, is within the ranking's size limit and the workspace has room behind
the lists in use; the workspace size itself is what it was."""
import os
import re

from conftest import ROOT


def _lib():
    from torchpq_amd import _lib
    return _lib, _lib.load()


def test_entry_points_are_declared_exported_and_bound():
    _lib_mod, lib = _lib()
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in ("tpq_ivfpq_scan_order", "tpq_ivfpq_scan_ordered"):
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in _lib_mod.SIGNATURES and hasattr(lib, name), name
    from torchpq_amd import kernels as K
    assert callable(K.ScanOrderHip) and hasattr(K.IVFPQTopkHip(m=64), "last_ordered")
    # validation comes before any HIP call
    assert lib.tpq_ivfpq_scan_order(None, None, None, 10, 8, 6, None, None, None, None) == -1
    assert "null pointer" in _lib_mod.last_error()


def _ordered(lib, nq, k=100, m=64, ds=2, n_probe=32, hint=31264, has_lut=0, residual=0, slots=1024, ws=None, n_split=1):
    if ws is None:
        ws = lib.tpq_ivfpq_scan_workspace_bytes(nq, k, n_split, m)
    return lib.tpq_ivfpq_scan_ordered(nq, k, n_split, m, ds, n_probe, hint, has_lut, 1, 0, residual, slots, ws)


def test_plan_orders_batches_of_more_than_one_round():
    _lib_mod, lib = _lib()
    assert lib.tpq_ivfpq_scan_route(10000, 100, 1, 64, 2, 32, 31264, 0, 1, 0, 0) == 16      # the headline call
    assert _ordered(lib, 10000) == 1
    assert _ordered(lib, 1025) == 1 and _ordered(lib, 1024) == 0        # one round of 1 024 slots: nothing to shorten
    assert _ordered(lib, 1025, slots=2048) == 0 and _ordered(lib, 2049, slots=2048) == 1
    assert _ordered(lib, 1000) == 0 and _ordered(lib, 256) == 0          # below the large-batch routes
    assert _ordered(lib, 20480) == 1 and _ordered(lib, 20481) == 0      # the pairwise ranking's limit
    assert _ordered(lib, 10000, k=300) == 1                              # k in (248, 504] rides the route too
    assert _ordered(lib, 10000, m=32, ds=4) == 1                         # the fp32 route of the short codes
    assert lib.tpq_ivfpq_scan_route(10000, 100, 1, 32, 4, 32, 31264, 0, 1, 0, 0) == 8
    assert _ordered(lib, 10000, k=600) == 0                              # the pools
    assert _ordered(lib, 10000, residual=1) == 0 and _ordered(lib, 10000, has_lut=1) == 0
    assert _ordered(lib, 0) == -1                                        # rejected like the route query


def test_order_needs_room_behind_the_lists_in_use():
    """the headline call uses one list of 64 keys per wave: flags + bands + 10 000 x 4 lists + their eviction words;
    the order takes three int32 arrays of 10 000, each rounded up to 256 bytes, behind them"""
    _lib_mod, lib = _lib()
    nq = 10000
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    used = 2 * align(nq * 4) + nq * 4 * 64 * 8 + align(nq * 4 * 4)
    need = used + 3 * align(nq * 4)
    assert _ordered(lib, nq, ws=need) == 1 and _ordered(lib, nq, ws=need - 1) == 0 and _ordered(lib, nq, ws=0) == 0
    assert need < lib.tpq_ivfpq_scan_workspace_bytes(nq, 100, 1, 64)


def test_workspace_size_is_unchanged():
    _lib_mod, lib = _lib()
    assert lib.tpq_ivfpq_scan_workspace_bytes(100, 100, 1, 64) == 2 * 512 + 100 * 16 * 128 * 8 + 6400
    assert lib.tpq_ivfpq_scan_workspace_bytes(100, 100, 1, 32) == 2 * 512 + 100 * 16 * 128 * 8 + 6400
    assert lib.tpq_ivfpq_scan_workspace_bytes(100, 100, 1, 24) == 2 * 512 + 100 * 4 * 128 * 8 + 1792
    assert lib.tpq_ivfpq_scan_workspace_bytes(100, 100, 4, 120) == 2 * 512 + 100 * 4 * 16 * 128 * 8 + 25600
    assert lib.tpq_ivfpq_scan_workspace_bytes(10000, 100, 1, 64) == 2 * 40192 + 10000 * 16 * 128 * 8 + 640000
