"""GPU: the inversion of the cell-major form (csrc/scan_cells.hip: cell_count_kernel, cell_scan_kernel,
cell_scatter_kernel) counts and scatters per workgroup, over a slice of kCellSlice consecutive queries in an LDS histogram
of n_cells ints, and falls back to one global atomic per pair past kCellLdsCells cells.  Kernel level, as
test_gpu_scan_cells_edges.py checks it: CellCandidatesHip with threshold -inf returns every live slot of every listed
probe -- first_probe <= p < n_probe_list[q] (clamped to the table's width), size > 0, start different from the previous
probe's -- exactly once, and `count` says how many.  The shapes are those at which the slices can go wrong: query counts
around every slice length the kernels are built or measured with, one cell under full contention, ragged lists with a
flagged query inside a slice, both sides of the LDS limit, a dirty workspace used twice."""
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "torchpq_amd", "csrc", "scan_cells.h")


def _constant(name):
    with open(_HEADER) as f:
        text = f.read()
    m = re.search(r"constexpr int %s = (\w+);" % name, text)
    value = m.group(1)
    if not value.isdigit():     # (a macro with a default: `#define NAME 256`)
        value = re.search(r"#define %s (\d+)" % value, text).group(1)
    return int(value)


SLICE = _constant("kCellSlice")
LDS_CELLS = _constant("kCellLdsCells")


def test_the_constants_read_from_the_header():
    assert 32 <= SLICE <= 1024 and 1024 <= LDS_CELLS <= 160 * 1024 // 4


# ---- problems and the oracle -------------------------------------------------------------------------------------------
def _build(seed, sizes, cells, npl, ds=2, holes=0.05):
    """cells of `sizes` slots, each with a start of its own (one unused slot behind it); probe table `cells` [nq, P]"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    cells = np.asarray(cells, np.int64)
    nq = cells.shape[0]
    cap = sizes + 1
    start = np.cumsum(cap) - cap
    n_slots = int(cap.sum())
    return dict(storage=rng.integers(0, 256, (16, n_slots, 4), dtype=np.uint8),
                codebook=(rng.standard_normal((64, ds, 256)) * 3).astype(np.float32),
                query=(rng.standard_normal((64 * ds, nq)) * 3).astype(np.float32),
                is_empty=(rng.random(n_slots) < holes).astype(np.uint8), cells=cells, npl=np.asarray(npl, np.int64),
                n_cells=len(sizes), n_slots=n_slots, cs=start[cells], sz=sizes[cells].copy())


def _listed(p, first):
    """per query the live slots of its listed probes"""
    nq, P = p["cells"].shape
    out = []
    for q in range(nq):
        slots = []
        for pr in range(first, int(np.clip(p["npl"][q], 0, P))):
            st, sz = p["cs"][q, pr], p["sz"][q, pr]
            if sz > 0 and not (pr > 0 and p["cs"][q, pr - 1] == st):
                slots.extend(range(st, st + sz))
        assert len(set(slots)) == len(slots), "the problem lists a cell twice at non-adjacent probes"
        out.append({s for s in slots if not p["is_empty"][s]})
    return out


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _capacity(want):
    capacity = max(64, (max(len(w) for w in want) + 63) // 64 * 64)
    assert capacity <= 4096
    return capacity


def _assert_exact(want, count, address, flags, flagged=()):
    assert sorted(np.nonzero(flags)[0].tolist()) == sorted(flagged)
    for q, w in enumerate(want):
        got = address[q, :count[q]].tolist()
        if q in flagged:
            assert count[q] == 0
            continue
        assert count[q] == len(w), (q, count[q], len(w))
        assert len(set(got)) == len(got), ("duplicates", q)
        assert set(got) == w, q


def _kernel_check(p, first, flagged=()):
    from torchpq_amd import kernels as K
    nq = p["cells"].shape[0]
    want = _listed(p, first)
    count, _, address, _, flags = (t.cpu().numpy() for t in K.CellCandidatesHip()(
        _T(p["storage"]), _T(p["query"]), _T(p["codebook"]), _T(p["cells"]), p["n_cells"], _T(p["cs"]), _T(p["sz"]),
        _T(p["npl"]), torch.full((nq,), -float("inf"), device=DEV), first_probe=first, capacity=_capacity(want),
        is_empty=_T(p["is_empty"])))
    assert (address[np.arange(address.shape[1])[None, :] >= count[:, None]] == -1).all()
    _assert_exact(want, count, address, flags, flagged)
    return count


def _perm_rows(rng, ids, nq, width):
    return np.stack([rng.permutation(ids)[:width] for _ in range(nq)])


def _sizes(rng, n):
    return rng.integers(1, 41, n)


# ---- query counts around the slice ---------------------------------------------------------------------------------------
# every slice length the kernels were measured with (128, 256, 512) is straddled, and two slices and one query of each
NQS = sorted({1, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1025, SLICE - 1, SLICE, SLICE + 1, 2 * SLICE + 1})


@pytest.mark.parametrize("first", [0, 4])
@pytest.mark.parametrize("nq", NQS)
def test_query_counts_around_the_slice(nq, first):
    rng = np.random.default_rng(1000 + nq)
    p = _build(nq + first, _sizes(rng, 24), _perm_rows(rng, np.arange(24), nq, 8), np.full(nq, 8), ds=1 + nq % 2)
    assert _kernel_check(p, first).min() > 0


# ---- one cell under full contention -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 4])
def test_one_cell_listed_by_600_queries_beside_cells_listed_by_one(first):
    """cell 0: one LDS counter and one global counter that every pair of every slice meets; cells 1 + q: one pair each"""
    nq = 600
    rng = np.random.default_rng(7)
    cells = np.zeros((nq, 8), np.int64)
    cells[:, :4] = 1 + nq + _perm_rows(rng, np.arange(8), nq, 4)     # (the probes of the threshold pass when first = 4)
    cells[np.arange(nq), 4 + np.arange(nq) % 2] = 0                   # the hot cell at probe 4 or 5 ...
    cells[np.arange(nq), 5 - np.arange(nq) % 2] = 1 + np.arange(nq)   # ... beside the query's own
    cells[:, 6:] = 1 + nq + 8 + _perm_rows(rng, np.arange(6), nq, 2)
    p = _build(8, _sizes(rng, 1 + nq + 14), cells, np.full(nq, 8))
    listed = np.bincount(cells[:, first:].reshape(-1), minlength=p["n_cells"])
    assert listed[0] == nq and (listed[1:1 + nq] == 1).all()
    _kernel_check(p, first)


# ---- ragged lists, repeats, empty cells, a flagged query inside a slice ------------------------------------------------------
@pytest.mark.parametrize("first", [0, 4])
def test_ragged_lists_with_a_flagged_query_inside_a_slice(first):
    nq = 2 * SLICE + 40
    rng = np.random.default_rng(11 + first)
    sizes = _sizes(rng, 30)
    sizes[[3, 17, 29]] = 0                                            # empty cells
    cells = _perm_rows(rng, np.arange(30), nq, 8)
    npl = rng.integers(0, 10, nq)                                     # (9 > the table's width: clamped)
    npl[[0, 5, SLICE - 1, SLICE, SLICE + 1, nq - 1]] = [0, first, 2, 0, 8, 8]     # several without a listed probe
    for q, pr in ((7, 4), (8, 3), (9, 5), (SLICE + 2, 6), (nq - 2, 4)):            # adjacent repeated probes
        cells[q, pr + 1] = cells[q, pr]
        npl[q] = 8
    cells[10, 5] = cells[10, 6] = cells[10, 4]                        # three in a row
    npl[10] = 8
    for q in (7, 8, 9, 10, SLICE + 2, nq - 2):     # a neighbour's cell over a probe keeps the row free of other repeats
        runs = [c for i, c in enumerate(cells[q]) if i == 0 or c != cells[q, i - 1]]
        assert len(set(runs)) == len(runs)
    bad = [SLICE // 2, SLICE + SLICE // 2 + 1]                        # in the middle of the first and the second slice
    npl[[bad[0] - 1, bad[0], bad[0] + 1, bad[1]]] = 8
    p = _build(12, sizes, cells, npl)
    p["query"][5, bad[0]] = float("nan")
    p["query"][77, bad[1]] = float("inf")
    want = _listed(p, first)
    assert sum(1 for w in want if not w) >= 4 and all(want[b] for b in bad) and want[bad[0] - 1] and want[bad[0] + 1]
    count = _kernel_check(p, first, flagged=bad)
    assert count[bad[0] - 1] > 0 and count[bad[0] + 1] > 0


# ---- cell counts: one, two, and both sides of the LDS histogram's limit -------------------------------------------------
@pytest.mark.parametrize("n_cells", [1, 2, LDS_CELLS, LDS_CELLS + 1])
def test_cell_counts_at_the_lds_limit(n_cells):
    """at kCellLdsCells the slices count in LDS, the last cell in the histogram's last int; one cell more and the pairs
    take one global atomic each"""
    nq = SLICE + 3
    rng = np.random.default_rng(n_cells)
    probed = sorted({c for c in (0, 1, n_cells // 2, n_cells - 3, n_cells - 2, n_cells - 1) if 0 <= c < n_cells})
    sizes = np.zeros(n_cells, np.int64)
    sizes[probed] = _sizes(rng, len(probed))
    ids = np.array(probed + ([n_cells // 3] if n_cells > 6 else []))     # (an empty cell among the probed ones)
    cells = _perm_rows(rng, ids, nq, len(ids))
    npl = rng.integers(0, len(ids) + 1, nq)
    npl[:6] = len(ids)
    p = _build(n_cells + 1, sizes, cells, npl, ds=1 + n_cells % 2)
    assert np.bincount(cells.reshape(-1), minlength=n_cells)[n_cells - 1] > 0
    assert _kernel_check(p, first=0).max() > 0


# ---- a dirty workspace, twice --------------------------------------------------------------------------------------------
def _raw_call(t, p, first, capacity, ws, threshold):
    """tpq_ivfpq_cell_candidates on the caller's workspace and fresh outputs"""
    from torchpq_amd._lib import ptr
    from torchpq_amd.kernels._common import call, metric_code
    nq, P = p["cells"].shape
    ds = p["codebook"].shape[1]
    count = torch.zeros(nq, device=DEV, dtype=torch.int32)
    keys = torch.zeros(nq, capacity, device=DEV, dtype=torch.int32)
    addr = torch.zeros(nq, capacity, device=DEV, dtype=torch.int32)
    band = torch.zeros(nq, device=DEV, dtype=torch.float32)
    flags = torch.zeros(nq, device=DEV, dtype=torch.int32)
    call("tpq_ivfpq_cell_candidates", t["storage"].device, ptr(t["storage"]), ptr(t["query"]), ptr(t["codebook"]), ds,
         metric_code("euclidean"), ptr(t["is_empty"]), ptr(t["cs"]), ptr(t["sz"]), ptr(t["npl"]), ptr(t["cells"]),
         p["n_cells"], first, ptr(threshold), p["n_slots"], nq, P, 64, capacity, ptr(count), ptr(keys), ptr(addr),
         ptr(band), ptr(flags), ptr(ws), ws.numel())
    torch.cuda.synchronize()
    return count.cpu().numpy(), (~addr).cpu().numpy().astype(np.int64), keys.cpu().numpy(), flags.cpu().numpy()


@pytest.mark.parametrize("slot_norms", [True, False])
def test_the_same_call_twice_on_a_workspace_of_0xa5(slot_norms):
    from torchpq_amd import _lib
    lib = _lib.load()
    nq, first = 2 * SLICE + 1, 4
    rng = np.random.default_rng(21)
    p = _build(22, _sizes(rng, 24), _perm_rows(rng, np.arange(24), nq, 8), rng.integers(0, 9, nq))
    want = _listed(p, first)
    capacity = _capacity(want)
    ws_bytes = (lib.tpq_ivfpq_cell_candidates_norms_workspace_bytes(nq, 8, p["n_cells"], first, p["n_slots"]) if slot_norms
                else lib.tpq_ivfpq_cell_candidates_workspace_bytes(nq, 8, p["n_cells"], first))
    ws = torch.full((ws_bytes,), 0xA5, device=DEV, dtype=torch.uint8)
    t = {key: _T(p[key]) for key in ("storage", "query", "codebook", "is_empty", "cs", "sz", "npl", "cells")}
    threshold = torch.full((nq,), -float("inf"), device=DEV)
    runs = [_raw_call(t, p, first, capacity, ws, threshold) for _ in range(2)]
    for count, address, keys, flags in runs:
        _assert_exact(want, count, address, flags)
    # the order inside a cell is not specified, so a query's entries may come in another order: equal as sets of
    # (value image, address)
    (c0, a0, k0, f0), (c1, a1, k1, f1) = runs
    assert np.array_equal(c0, c1) and not f0.any() and not f1.any()
    for q in range(nq):
        assert sorted(zip(k0[q, :c0[q]].tolist(), a0[q, :c0[q]].tolist())) == \
               sorted(zip(k1[q, :c1[q]].tolist(), a1[q, :c1[q]].tolist())), q
