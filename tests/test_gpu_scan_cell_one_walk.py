"""GPU: the threshold form's inversion (csrc/scan_cells.hip, launch_cell_threshold): one count / scan / scatter walk
fills pass B's view (every listed probe) and pass A's (the listed probes p < T) while two LDS histograms fit
(n_cells <= kCellLdsCells / 2); beyond, and beyond kCellLdsCells, each view has its own walk.  Both views are read from
the kept workspace of a whole search (the layout: csrc/scan_cells.h, cell_fill_extras and cell_fill_thr) and compared,
per cell, with a Python listing: the multiset of queries, and the extent of every listed cell.  The search's results
are compared with the reference-layout kernel as everywhere.
The form is a route of batches of 1 024 queries and more, so the query counts around a slice are 8 slices + 127, 128,
129 and 10 slices + 1 here, not 127, 128, 129 themselves."""
import numpy as np
import pytest
import torch

from test_gpu_scan_cell_inversion import LDS_CELLS, SLICE
from test_gpu_scan_cell_threshold import SIZES
from test_gpu_scan_cells import DEV, _problem, _search
from test_scan_cell_maxima_cpu import T

pytestmark = pytest.mark.gpu

N_PROBE = 12


def _views(p, scan, k):
    """(cell_off, pairs, cell_st, cell_sz) of pass B's and of pass A's view, from the kept workspace"""
    from torchpq_amd._lib import load
    ws = scan.last_workspace
    nq, n_probe = p["cells"].shape
    nc, n_slots = p["n_cells"], p["n_slots"]
    align = lambda n: (n + 255) // 256 * 256  # noqa: E731
    lists = lambda ch: 2 * align(nq * 4) + nq * ch * 512 + align(nq * ch * 4)  # noqa: E731
    extras = load().tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, nc, 4)
    chunks = next(ch for ch in (16, 8) if (k + 63) // 64 < ch and scan.last_workspace_bytes >= lists(ch) + extras)
    arr = lambda off, n: ws[off:off + 4 * n].view(torch.int32).cpu().numpy()  # noqa: E731
    cells, cells1 = align(nc * 4), align((nc + 1) * 4)
    o = lists(chunks) + 256 + 4 * align(nq * 4) + cells           # (params, thr, qscale, qnorm, cnt, hist)
    off_b, st_b, sz_b = arr(o, nc + 1), arr(o + 2 * cells1, nc), arr(o + 2 * cells1 + cells, nc)
    t0 = lists(chunks) + extras + align(n_slots * 4)
    pairs_b = arr(t0, nq * n_probe)
    o = t0 + align(nq * n_probe * 4) + cells                      # (pass B's pairs, pass A's hist)
    off_a, st_a, sz_a = arr(o, nc + 1), arr(o + 2 * cells1, nc), arr(o + 2 * cells1 + cells, nc)
    pairs_a = arr(o + 2 * cells1 + 2 * cells, nq * min(T, n_probe))
    return (off_b, pairs_b, st_b, sz_b), (off_a, pairs_a, st_a, sz_a)


def _listing(p, flagged, p_hi):
    """per cell the sorted queries that list it at a probe p < p_hi: listed = inside the query's probe count, not
    empty, not the previous probe's cell again; a flagged query lists nothing"""
    cells, npl = p["cells"].cpu().numpy(), p["npl"].cpu().numpy()
    sizes = p["sizes"].cpu().numpy()
    out = [[] for _ in range(p["n_cells"])]
    for q in range(cells.shape[0]):
        if q in flagged:
            continue
        for pr in range(min(int(npl[q]), cells.shape[1], p_hi)):
            c = cells[q, pr]
            if sizes[c] > 0 and not (pr > 0 and cells[q, pr - 1] == c):
                out[c].append(q)
    return [sorted(x) for x in out]


def _check_views(p, k=10, flagged=()):
    """both views against the listing, and WHICH walk filled them: the library counts the count / scan / scatter chains
    it launches (tpq_ivfpq_scan_cell_inversions) -- one for the call while two LDS histograms fit, two beyond"""
    from torchpq_amd._lib import load
    before = load().tpq_ivfpq_scan_cell_inversions()
    got, scan = _search(p, k)
    assert scan.last_cell_threshold() is True
    assert load().tpq_ivfpq_scan_cell_inversions() - before == (1 if p["n_cells"] <= LDS_CELLS // 2 else 2)
    start, sizes = p["start"].cpu().numpy(), p["sizes"].cpu().numpy()
    for (off, pairs, st, sz), p_hi in zip(_views(p, scan, k), (N_PROBE, T)):
        want = _listing(p, set(flagged), p_hi)
        assert off[0] == 0 and off[-1] == sum(len(w) for w in want)
        for c, w in enumerate(want):
            assert sorted(pairs[off[c]:off[c + 1]].tolist()) == w, (p_hi, c)
            if w:
                assert (st[c], sz[c]) == (start[c], sizes[c]), (p_hi, c)
    ref, _ = _search(p, k, cells=False, packed=False)
    ok = torch.ones(got[0].shape[0], dtype=torch.bool, device=DEV)
    ok[list(flagged)] = False
    assert torch.equal(got[0][ok].view(torch.int32), ref[0][ok].view(torch.int32))
    assert torch.equal(got[1], ref[1])
    return scan


@pytest.mark.parametrize("nq", [1024, 8 * SLICE + 127, 8 * SLICE + 128, 8 * SLICE + 129, 10 * SLICE + 1])
def test_both_views_around_the_slice(nq):
    """ragged probe counts (0, 1, T - 1, T, T + 1 among them), probes repeated across the pass-A boundary, and a flagged
    query (a NaN component) in the middle of a slice"""
    p = _problem(nq, nq, 16, N_PROBE, 1 + nq % 2, sizes=SIZES * 2)
    p["npl"][:8] = torch.tensor([0, 1, T - 1, T, T + 1, N_PROBE, 2, N_PROBE], device=DEV)
    q = torch.arange(nq, device=DEV)
    p["cells"][q % 5 == 0, T] = p["cells"][q % 5 == 0, T - 1]
    p["cells"][q % 5 == 1, T - 1] = p["cells"][q % 5 == 1, T - 2]
    bad = SLICE + SLICE // 2
    p["query"][3, bad] = float("nan")
    p["npl"][bad - 1:bad + 2] = N_PROBE
    _check_views(p, flagged=[bad])


def test_one_cell_listed_by_600_queries_beside_cells_listed_by_one():
    """cell 0 meets every slice's LDS counter and one global counter per view, before T for half of its queries and
    behind it for the others; cells 16 + q are listed by query q alone, at probe 1 or T + 1"""
    nq, hot = 1024, 600
    sizes = [640] + (SIZES * 2)[1:] + [40] * hot
    p = _problem(77, nq, 16 + hot, N_PROBE, 2, sizes=sizes, ragged=False)
    g = torch.Generator(device=DEV)
    g.manual_seed(78)
    p["cells"] = (1 + torch.rand(nq, 15, generator=g, device=DEV).argsort(1)[:, :N_PROBE]).contiguous()
    q = torch.arange(hot, device=DEV)
    p["cells"][q, torch.where(q % 2 == 0, 2, T + 2)] = 0
    p["cells"][q, torch.where(q % 2 == 0, T + 1, 1)] = 16 + q
    p["hint"] = N_PROBE * 600
    _check_views(p)


@pytest.mark.parametrize("n_cells", [LDS_CELLS // 2, LDS_CELLS // 2 + 1, LDS_CELLS, LDS_CELLS + 1])
def test_cell_counts_at_the_limits(n_cells):
    """two LDS histograms up to kCellLdsCells / 2 cells, the last cell in the last int of each; one cell more and each view
    has its own walk; beyond kCellLdsCells the wide kernels.  Sixteen cells hold slots, the last cell among them"""
    nq = 1300
    live = [0, 1, 2, n_cells // 3, n_cells // 2 - 1, n_cells // 2, n_cells - 3, n_cells - 2, n_cells - 1]
    live = sorted(set(live + list(range(5, 5 + 16 - len(set(live))))))
    assert len(live) == 16
    sizes = np.zeros(n_cells, np.int64)
    sizes[live] = (SIZES * 2)[:16]
    p = _problem(n_cells, nq, 16, N_PROBE, 2, sizes=[1] * 16)   # (queries, codebook, probe counts; the cells: below)
    g = torch.Generator(device=DEV)
    g.manual_seed(n_cells)
    st = torch.from_numpy(np.cumsum(sizes + 5) - (sizes + 5)).to(DEV)
    n_slots = int((sizes + 5).sum())
    ids = torch.tensor(live + [4], device=DEV)           # (an empty cell among the probed ones)
    p.update(sizes=torch.from_numpy(sizes).to(DEV), start=st, n_cells=n_cells, n_slots=n_slots,
             storage=torch.randint(0, 256, (16, n_slots, 4), generator=g, device=DEV, dtype=torch.uint8),
             is_empty=(torch.rand(n_slots, generator=g, device=DEV) < 0.05).to(torch.uint8),
             cells=ids[torch.rand(nq, 17, generator=g, device=DEV).argsort(1)[:, :N_PROBE]].contiguous(),
             hint=N_PROBE * 1000)
    p.pop("packed", None)
    scan = _check_views(p)
    assert scan.last_cell_major() is True


def test_a_workspace_of_0xa5_twice(monkeypatch):
    """every buffer the wrapper allocates pre-filled with 0xa5, two searches: both views are written whole before they
    are read, whatever the workspace held"""
    from guarded_alloc import run_guarded
    from torchpq_amd import kernels as K
    p = _problem(91, 1100, 16, N_PROBE, 2, sizes=SIZES * 2)
    p["packed"] = K.PackCodesHip()(p["storage"])

    def go():
        _check_views(p)
        _check_views(p)
        return True
    assert all(run_guarded(go, fills=(0xA5,), monkeypatch=monkeypatch).values())
