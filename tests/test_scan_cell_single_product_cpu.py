"""CPU: the single-product selection key of the cell-major scan's threshold form (csrc/scan_cells.hip, `The single-product
key`) in float64 -- tests/cell_single_product_model.py over the input families of tests/scan_cells_oracle.py.  The key
stays within delta1_q of the exact value for every slot, ds 1 and 2, both metrics, subnormal pieces kept and flushed
(`coherent_lo` and its kin put the low pieces, which the key drops, where they count); the dropped products stay within
the per-sub-quantizer bound; the band from the packed maxima is never below the band from the exact ones; the header's
lines, written out again, sum to the constant in the source; the switch and the report are exported."""
import os
import re

import numpy as np
import pytest

import cell_single_product_model as S
import scan_cells_oracle as O
from conftest import ROOT

N_SLOTS = 200
CASES = [(f, ds, metric) for f in O.FAMILIES for ds in (1, 2) for metric in O.METRICS]


def _inputs(name, ds):
    nq = 64 if name == "one_subq" else 8
    return O.family(name, ds, nq, N_SLOTS, seed=1)


@pytest.mark.parametrize("name,ds,metric", CASES)
def test_key_is_within_delta1_of_exact(name, ds, metric):
    cb, q, codes = _inputs(name, ds)
    for flush in (False, True):
        r = S.evaluate1(q, cb, codes, metric, flush=flush)
        for packed in (False, True):
            d1 = S.delta1_q(q, cb, packed=packed, flush=flush)
            ratio = (np.abs(r["key"] - r["exact"]) + r["tol"]) / d1[:, None]
            assert np.isfinite(ratio).all()
            assert ratio.max() <= 1.0, (name, ds, metric, flush, packed, ratio.max())


@pytest.mark.parametrize("name,ds,metric", CASES)
def test_dropped_products_are_within_their_bound(name, ds, metric):
    """the query's own term alone, without the factor 1.25 and the other lines"""
    cb, q, codes = _inputs(name, ds)
    r = S.evaluate1(q, cb, codes, metric)
    XH, XL = S.piece_maxima(r["p"])
    bound = S.dropped_bound(r["p"], XH, XL)
    assert (np.abs(r["dropped"]) <= bound[:, None] * (1 + 1e-12)).all()
    if name == "coherent_lo" and metric == "euclidean":   # (the family is there to make the term count: it is not slack)
        assert (np.abs(r["dropped"]).max(1) >= 0.05 * bound).all()


@pytest.mark.parametrize("name", O.FAMILIES)
@pytest.mark.parametrize("ds", (1, 2))
def test_packed_maxima_only_loosen_the_band(name, ds):
    cb, q, _ = _inputs(name, ds)
    p = S.pieces(q, cb)
    XH, XL = S.piece_maxima(p)
    PH, PL = S.packed_maxima(XH, XL)
    assert (PH >= XH).all() and (PL >= XL).all()
    assert (PH <= XH.reshape(32, 2).max(1).repeat(2) * 1.0001 * (1 + 2.0 ** -7)).all()
    assert (S.delta1_q(q, cb, packed=True) >= S.delta1_q(q, cb, packed=False)).all()


def test_round_up_16():
    v = np.array([1.0, 1.0 + 2.0 ** -20, 4096.0, 5793.3, 2.0 ** -30, 11585.2])
    r = S.round_up_16(v)
    assert (r >= v * 1.0001 * (1 - 2.0 ** -24)).all() and (r <= v * 1.0001 * (1 + 2.0 ** -7)).all()
    assert ((r.astype(np.float32).view(np.uint32) & 0xffff) == 0).all()


@pytest.mark.parametrize("ds", (1, 2))
def test_delta1_rel_is_the_headers_sum(ds):
    """the header's lines for N = D MFMA terms, written out again from its text, and the constants in the source"""
    D, m = 64.0 * ds, 64
    N = D
    lines = [
        (2.03 * 2.0 ** -22 + 1.003 * N * 2.0 ** -23) / 2 + 1.01 * np.sqrt(D) * 2.0 ** -26,   # residues, accumulation
        (D + 1) * 2.0 ** -24,                                                               # the norm chains
        14 * 2.0 ** -24,                                                                    # |x|^2 from the pieces
        2.0 ** -22,                                                                         # the two subtractions
        1.001 * (m + ds + 2) * 2.0 ** -24,                                                  # the exact chain
    ]
    assert abs(S.delta1_rel(ds) - 1.25 * sum(lines)) <= 1e-12 * sum(lines)
    assert S.delta1_rel(ds) < O.delta_rel(ds)          # (a third of the accumulated terms, one product less dropped)
    src = open(os.path.join(ROOT, "torchpq_amd", "csrc", "scan_cells.hip")).read()
    body = re.search(r"float cell_delta1_rel\(int ds\) \{(.*?)\n\}", src, re.S).group(1)
    for token in ("N = D", "2.03 * 4 * u", "1.003 * N * 2 * u", "1.01 * std::sqrt(D) * u / 4", "(D + 1) * u", "14 * u",
                  "4 * u", "1.001 * (64 + ds + 2) * u", "1.25 * sum"):
        assert token in body, token
    # cell_delta_rel stays as it is
    old = re.search(r"float cell_delta_rel\(int ds\) \{(.*?)\n\}", src, re.S).group(1)
    assert "N = 3.0 * D" in old and "3.03 * 4 * u" in old
    # the seed kernel applies 1.25 to the query's own term as well, upwards
    assert "1.25f * 1.0001f * t" in src


def test_switch_and_report_are_exported():
    from torchpq_amd import _lib
    lib = _lib.load()
    assert lib.tpq_ivfpq_scan_use_cell_single_product(0) == 1      # default on
    assert lib.tpq_ivfpq_scan_use_cell_single_product(1) == 0
    assert lib.tpq_ivfpq_scan_use_cell_single_product(1) == 1
    assert lib.tpq_ivfpq_scan_last_cell_products() in (0, 1, 3)
    from torchpq_amd.index import IVFPQIndex
    assert IVFPQIndex.use_cell_single_product is True
