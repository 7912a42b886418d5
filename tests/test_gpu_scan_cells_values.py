"""GPU: the VALUES of the cell-major candidate pass (cell_cand_kernel, csrc/scan_cells.hip) against the float64 model of
tests/scan_cells_oracle.py.  The admission test and the finish kernel's cut are right only while the fp16-split
matrix-core value stays within delta_q of the exact one; on random data a kernel that loses a whole product of the
split still does, so the families here put the low pieces where they count (the oracle's docstrings say how).  Every
case returns every live listed slot (threshold -inf) and compares slot by slot:

  |value - exact| <= band / 2         the kernel's own promise (band = 2 delta_q);
  |value - model| <= tol              the rounding allowance of the documented arithmetic for that slot (not on `wide`,
                                      where the hardware may flush a subnormal piece or keep it);
  band / 2 >= delta_rel B^2           the kernel uses no smaller delta than it documents;

then repeats the call with a finite threshold and checks the containment conditions of test_gpu_scan_cells.py.

TPQ_CELL_VALUE_ERROR_JSON=<path> records the largest observed ratios per case in that file (profiles/
cell_value_error.json is such a record; the ratios are records, the thresholds are the derived ones above)."""
import json
import os

import numpy as np
import pytest
import torch

import scan_cells_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = np.array([1, 31, 32, 33, 64, 65, 33])     # the tile is 32 slots
GAP = 3
FIRST = 1
CAPACITY = 320
CASES = [(f, ds, metric) for f in O.FAMILIES for ds in (1, 2) for metric in O.METRICS]


def _record(key, exact_ratio, model_ratio):
    path = os.environ.get("TPQ_CELL_VALUE_ERROR_JSON")
    if not path:
        return
    doc = json.load(open(path)) if os.path.exists(path) else {}
    doc.setdefault("what", "largest |value - exact| / delta_q and |value - model| / tol over every returned slot of "
                           "tests/test_gpu_scan_cells_values.py, per family, ds and metric (MI355X); records, not bounds")
    doc.setdefault("cases", {})[key] = {"value_minus_exact_over_delta_q": float(exact_ratio),
                                        "value_minus_model_over_tol": None if model_ratio is None else float(model_ratio)}
    with open(path, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")


def _layout(name, ds):
    """cells of 1, 31, 32, 33, 64, 65 and 33 slots with gaps between them, tombstones, ragged probe lists"""
    nq = 64 if name == "one_subq" else 96
    n_cells = len(SIZES)
    cap = SIZES + GAP
    start = np.cumsum(cap) - cap
    n_slots = int(cap.sum())
    cb, q, codes = O.family(name, ds, nq, n_slots, seed=2)
    rng = np.random.default_rng([3, O.FAMILIES.index(name), ds])
    emp = (rng.random(n_slots) < 0.05).astype(np.uint8)
    cells = np.stack([rng.permutation(n_cells) for _ in range(nq)]).astype(np.int64)
    npl = rng.integers(0, n_cells + 1, nq).astype(np.int64)
    npl[:6] = [0, 1, 2, n_cells, n_cells, n_cells - 1]
    live = np.zeros((nq, n_slots), bool)
    for qi in range(nq):
        for c in cells[qi, FIRST:npl[qi]]:
            live[qi, start[c]:start[c] + SIZES[c]] = True
    live &= emp[None, :] == 0
    assert live.sum(1).max() <= CAPACITY
    return dict(cb=cb, q=q, codes=codes, emp=emp, cells=cells, npl=npl, start=start, live=live, nq=nq,
                n_cells=n_cells, n_slots=n_slots)


def _run(L, threshold, distance):
    from torchpq_amd import kernels as K
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    out = K.CellCandidatesHip()(
        T(O.storage_of(L["codes"])), T(L["q"]), T(L["cb"]), T(L["cells"]), L["n_cells"], T(L["start"][L["cells"]]),
        T(SIZES[L["cells"]]), T(L["npl"]), T(threshold.astype(np.float32)), first_probe=FIRST, capacity=CAPACITY,
        is_empty=T(L["emp"]), distance=distance)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _sets(L, count, address, flags):
    """flags 0, counts in range, no duplicates, nothing but live listed slots, -1 behind the count -> the address lists"""
    assert not flags.any()
    got = []
    for qi in range(L["nq"]):
        assert 0 <= count[qi] <= CAPACITY
        g = address[qi, :count[qi]]
        assert (address[qi, count[qi]:] == -1).all()
        assert len(np.unique(g)) == len(g), "duplicates"
        assert ((g >= 0) & (g < L["n_slots"])).all() and L["live"][qi, g].all()
        got.append(g)
    return got


@pytest.mark.parametrize("name,ds,metric", CASES)
def test_values_against_the_model(name, ds, metric):
    L = _layout(name, ds)
    r = O.evaluate(L["q"], L["cb"], L["codes"], metric)
    nq, live = L["nq"], L["live"]
    count, values, address, band, flags = _run(L, np.full(nq, -np.inf), metric)
    got = _sets(L, count, address, flags)
    # the kernel uses no smaller delta than it documents
    B = O.bound_B(L["q"], L["cb"])
    assert (band.astype(np.float64) / 2 >= O.delta_rel(ds) * B * B).all()
    worst_exact = worst_model = 0.0
    for qi in range(nq):
        g, v = got[qi], values[qi, :count[qi]].astype(np.float64)
        assert count[qi] == live[qi].sum() and set(g.tolist()) == set(np.nonzero(live[qi])[0].tolist())
        if not len(g):
            continue
        assert np.isfinite(v).all()
        e_exact = np.abs(v - r["exact"][qi, g]) / (band[qi] / 2.0)
        e_model = np.abs(v - r["model"][qi, g]) / r["tol"][qi, g]
        worst_exact, worst_model = max(worst_exact, e_exact.max()), max(worst_model, e_model.max())
    print(f"{name} ds={ds} {metric}: |value - exact| / delta_q <= {worst_exact:.4g}, "
          f"|value - model| / tol <= {worst_model:.4g}")
    _record(f"{name}-ds{ds}-{metric}", worst_exact, None if name == "wide" else worst_model)
    assert worst_exact <= 1.0
    if name != "wide":
        assert worst_model <= 1.0

    # a finite threshold: the fp32 image, rounded towards -inf, of the exact value of the query's 10th best listed slot
    # (of its worst when it lists fewer; -inf when it lists none): that slot and every better one must come back
    masked = np.where(live, r["exact"], -np.inf)
    order = np.sort(masked, 1)[:, ::-1]
    n_live = live.sum(1)
    pick = order[np.arange(nq), np.clip(np.minimum(n_live, 10) - 1, 0, None)]
    tau = pick.astype(np.float32)
    tau = np.where(tau.astype(np.float64) > pick, np.nextafter(tau, np.float32(-np.inf)), tau).astype(np.float32)
    assert (tau.astype(np.float64) <= pick).all()
    count, values, address, band, flags = _run(L, tau, metric)
    got = _sets(L, count, address, flags)
    for qi in range(nq):
        g = got[qi]
        must = set(np.nonzero(live[qi] & (r["exact"][qi] >= np.float64(tau[qi])))[0].tolist())
        assert len(must) >= min(n_live[qi], 10)
        assert must <= set(g.tolist())
        assert (r["exact"][qi, g] >= np.float64(tau[qi]) - np.float64(band[qi])).all()
        assert band[qi] > 0
        v = values[qi, :count[qi]].astype(np.float64)
        assert (np.abs(v - r["exact"][qi, g]) <= band[qi] / 2.0).all()
