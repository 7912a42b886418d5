"""The kept state of the cell-major scan (csrc/scan_cells.hip, `The kept state`), the parts that need no GPU: the two
exports and the header's define, the size function against the layout the tests restate, the numpy restatement of the
split codebook (tests/cell_kept_cases.py: what tests/test_gpu_scan_cell_kept.py compares the state's image with), the
argument check of the new entry point, and the registration of its guarded-buffer cases."""
import os

import numpy as np

import cell_kept_cases as ck
import guarded_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from torchpq_amd import _lib
    return _lib.load()


def test_exports_and_header():
    from torchpq_amd import _lib
    lib = _lib.load()
    for name in ("tpq_ivfpq_search_fused_cells_kept", "tpq_ivfpq_cell_kept_bytes", "tpq_ivfpq_scan_cell_inversions"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert lib.tpq_ivfpq_scan_cell_inversions() >= 0
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    assert "#define TPQ_HAS_IVFPQ_CELL_KEPT 1" in header and "#define TPQ_VERSION 500 " in header
    for name in ("tpq_ivfpq_search_fused_cells_kept(", "tpq_ivfpq_cell_kept_bytes("):
        assert name in header
    assert lib.tpq_version() == 500


def test_size_function():
    lib = _lib()
    for n_slots in (1, 63, 64, 65, 8815, 1 << 20, 100_000_000):
        for ds in (1, 2):
            assert lib.tpq_ivfpq_cell_kept_bytes(n_slots, ds) == ck.kept_bytes(n_slots, ds)
    assert lib.tpq_ivfpq_cell_kept_bytes(1 << 20, 2) == 256 + 131072 + (4 << 20)
    for n_slots, ds in ((0, 2), (-1, 1), (100, 0), (100, 3), (100, 4)):
        assert lib.tpq_ivfpq_cell_kept_bytes(n_slots, ds) == 0


def test_the_restated_split():
    """layout and arithmetic of the codebook image: per entry the ds hi pieces, then the ds lo pieces; the largest scaled
    entry in [2^12, 2^13); hi + lo within 2^-22 of the scaled entry, or 2^-24 absolute below the fp16 normal range"""
    rng = np.random.default_rng(0)
    for ds in (1, 2):
        cb = (rng.standard_normal((64, ds, 256)) * 3).astype(np.float32)
        cb[5, 0, 9] = 0.0
        cb[6, ds - 1, 200] = 1e-9
        img = ck.split_image(cb)
        assert img.dtype == np.uint16 and img.shape == (64, 256, 2 * ds)
        assert img.nbytes == ck.kept_bytes(0, ds) - 256
        sx = ck.scale(cb)
        ys = cb * sx
        assert 2.0 ** 12 <= np.abs(ys).max() < 2.0 ** 13 and np.log2(sx) == np.round(np.log2(sx))
        pieces = img.view(np.float16).astype(np.float64)
        for e in range(ds):
            hi, lo = pieces[:, :, e], pieces[:, :, ds + e]
            want = ys[:, e, :].astype(np.float64)
            assert np.array_equal(hi, ys[:, e, :].astype(np.float16).astype(np.float64))
            assert np.all(np.abs(hi + lo - want) <= np.maximum(np.abs(want) * 2.0 ** -22, 2.0 ** -24))
        assert img[5, 9, 0] == 0 and img[5, 9, ds] == 0


def test_the_entry_point_checks_its_arguments_before_it_launches():
    """null pointers are rejected as tpq_ivfpq_search_fused_cells rejects them, whatever the state"""
    from torchpq_amd import _lib
    lib = _lib.load()
    rc = lib.tpq_ivfpq_search_fused_cells_kept(None, None, None, None, 2, 0, None, None, None, None, None, None, None,
                                               None, 1000, 10, 8, 64, 10, 1, None, 0, None, 0, None, 8, None, 0, 1, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    rc = lib.tpq_ivfpq_search_fused_cells_kept(None, None, None, None, 2, 0, None, None, None, None, None, None, None,
                                               None, 1000, 10, 8, 64, 10, 1, None, 0, None, 0, None, 8, 264, 1 << 20, 1,
                                               None)
    assert rc == -1 and "16-byte aligned" in _lib.last_error()


def test_the_guarded_cases_are_registered():
    assert sorted(guarded_cases.CASES["tpq_ivfpq_search_fused_cells_kept"]) == sorted(ck.CASE_SYMBOLS)
    import test_gpu_guarded_buffers as gpu
    assert set(ck.CASE_SYMBOLS) <= set(gpu.BUILDERS) and set(ck.CASE_SYMBOLS) <= set(guarded_cases.CASE_IDS)


def test_the_index_switch():
    from torchpq_amd.index import IVFPQIndex
    from torchpq_amd.index.graphed import GraphedSearch
    assert IVFPQIndex.use_cell_kept is True and "use_cell_kept" in GraphedSearch.KNOBS
