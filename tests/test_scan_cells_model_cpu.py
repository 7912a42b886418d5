"""CPU: the standing of tests/scan_cells_oracle.py, the model the GPU tests of the cell-major candidate values lean on
(test_gpu_scan_cells_values.py).  The reference alone must meet what those tests assert of the kernel: the model stays
within delta_q of the exact value on every input family, with subnormal pieces kept and flushed; delta_rel is what the
header of csrc/scan_cells.hip documents; and a plain fp32 emulation of the accumulation stays within the per-slot
tolerance of the model."""
import os
import re

import numpy as np
import pytest

import scan_cells_oracle as O
from conftest import ROOT

N_SLOTS = 200
CASES = [(f, ds, metric) for f in O.FAMILIES for ds in (1, 2) for metric in O.METRICS]


def _inputs(name, ds):
    nq = 64 if name == "one_subq" else 8
    return O.family(name, ds, nq, N_SLOTS, seed=1)


@pytest.mark.parametrize("name,ds,metric", CASES)
def test_model_is_within_delta_of_exact(name, ds, metric):
    cb, q, codes = _inputs(name, ds)
    for flush in (False, True):
        r = O.evaluate(q, cb, codes, metric, flush=flush)
        ratio = np.abs(r["model"] - r["exact"]) / r["delta"][:, None]
        assert np.isfinite(ratio).all()
        assert ratio.max() <= 1.0, (name, ds, metric, flush, ratio.max())


@pytest.mark.parametrize("name,ds,metric", CASES)
def test_fp32_emulation_is_within_tol_of_model(name, ds, metric):
    cb, q, codes = _inputs(name, ds)
    r = O.evaluate(q, cb, codes, metric, emulate=True)
    assert (np.abs(r["emu"] - r["exact"]) <= r["delta"][:, None]).all()
    if name != "wide":   # (whether a subnormal piece is flushed is the hardware's to choose: only delta_q applies)
        ratio = np.abs(r["emu"] - r["model"]) / r["tol"]
        assert ratio.max() <= 1.0, (name, ds, metric, ratio.max())


@pytest.mark.parametrize("ds", (1, 2))
def test_delta_rel_is_the_headers_sum(ds):
    """the header's lines, written out again here from its text, and the constants of cell_delta_rel in the source"""
    D, N, m = 64.0 * ds, 3 * 64.0 * ds, 64
    lines = [
        (3.03 * 2.0 ** -22 + 1.003 * N * 2.0 ** -23) / 2 + 1.01 * np.sqrt(D) * 2.0 ** -26,   # products, accumulation
        (D + 1) * 2.0 ** -24,                                                               # the norm chains
        14 * 2.0 ** -24,                                                                    # |x|^2 from the pieces
        2.0 ** -22,                                                                         # the two subtractions
        1.001 * (m + ds + 2) * 2.0 ** -24,                                                  # the exact chain
    ]
    assert O.delta_rel(ds) >= sum(lines)
    assert abs(O.delta_rel(ds) - 1.25 * sum(lines)) <= 1e-12 * sum(lines)
    src = open(os.path.join(ROOT, "torchpq_amd", "csrc", "scan_cells.hip")).read()
    body = re.search(r"float cell_delta_rel\(int ds\) \{(.*?)\n\}", src, re.S).group(1)
    for token in ("3.03 * 4 * u", "1.003 * N * 2 * u", "1.01 * std::sqrt(D) * u / 4", "(D + 1) * u", "14 * u", "4 * u",
                  "1.001 * (64 + ds + 2) * u", "1.25 * sum"):
        assert token in body, token


def test_split_and_scales():
    y = np.array([4096.0, 4097.0, 8191.75, 1.0 + 2.0 ** -12, 3e-6, -5000.3], np.float32)
    h, l = O.split(y)
    assert np.array_equal(h, y.astype(np.float16).astype(np.float64))
    assert (np.abs(y - h - l) <= 2.0 ** -22 * np.abs(y) + 2.0 ** -14).all()
    hf, lf = O.split(y, flush=True)
    assert hf[4] == 0.0 and h[4] != 0.0
    for v, e in ((1.0, 12), (1.999, 12), (2.0, 11), (0.75, 13), (2.0 ** 40 * 1.5, -28), (2.0 ** -40, 52)):
        assert O.scale_of(v) == 2.0 ** e and 2.0 ** 12 <= v * O.scale_of(v) < 2.0 ** 13
    assert O.ulp_fp16(4096.0) == 4.0 and O.ulp_fp16(1024.0) == 1.0 and O.ulp_fp16(4095.0) == 2.0


def test_families_are_what_they_say():
    for ds in (1, 2):
        cb, q, _ = O.family("coherent_lo", ds, 8, N_SLOTS, seed=1)
        for a, s in ((cb, O.scale_of(np.abs(cb).max())), (q, O.scale_of(np.abs(q).max(0))[None, :])):
            h, l = O.split((a * s).astype(np.float32))
            r = l / O.ulp_fp16(h)
            assert (a > 0).all() and (r > 0.04).all() and (r < 0.46).all()
            assert len(np.unique(l)) > 20                        # (identical low pieces would hide a swap)
        cb, q, _ = O.family("one_subq", ds, 64, N_SLOTS, seed=1)
        nz = (q != 0).reshape(64, ds, 64)
        assert all(nz[j, :, j].all() and nz[:, :, j].sum() == ds for j in range(64))
        for name in ("scaled", "scaled_rev"):
            cb, q, _ = O.family(name, ds, 8, N_SLOTS, seed=1)
            for a in (np.abs(cb).max(), *np.abs(q).max(0)):
                assert -O.MAX_EXP <= np.frexp(a)[1] - 1 <= O.MAX_EXP
        cb, q, codes = O.family("near", ds, 8, N_SLOTS, seed=1)
        r = O.evaluate(q, cb, codes, "euclidean")
        assert (np.abs(r["exact"]).min(1) < 1e-3 * r["delta"]).all()   # a value close to 0 under a large B^2
        a, b, c = O.family("wide", ds, 8, N_SLOTS, seed=1)
        a2, b2, c2 = O.family("wide", ds, 8, N_SLOTS, seed=1)
        assert np.array_equal(a, a2) and np.array_equal(b, b2) and np.array_equal(c, c2)
        assert np.abs(a).min() < 2.0 ** -25 and np.abs(a).max() > 0.5
