"""GPU: the inversion and the dispatch of the cell-major form (csrc/scan_cells.hip: histogram, prefix scan, scatter, the
search for a block's cell; scan.hip: the form's stages) at the shapes where they can go wrong -- more than 1 024 cells,
runs of unprobed cells, more than 64 listed probes, a probe repeated across the P0 - 1 | P0 boundary, void probes,
groups of 31 / 32 / 33 queries, cells of 31 / 32 / 33 slots, the scale limits, a workspace used again.

Two kinds of check:
  kernel level  CellCandidatesHip with threshold -inf returns every live listed slot: set equality against a numpy
                enumeration of what fetch_probes (csrc/scan_shared.h) lists -- probes first_probe <= p < n_probe_list[q]
                (clamped to the table's width), size > 0, start different from the previous probe's;
  end to end    _check of test_gpu_scan_cells.py: the form ran and equals the reference-layout kernel bit for bit.
The problems are built in numpy (nothing here needs the GPU until the call), so the host rule is asserted first."""
import numpy as np
import pytest
import torch

from test_gpu_scan_cells import DEV, P0, _check, _problem, _search

pytestmark = pytest.mark.gpu


# ---- problems ----------------------------------------------------------------------------------------------------------
def _build(seed, sizes, cells, npl, ds=2, gap=1, holes=0.05, codebook=None, query=None):
    """numpy problem over cells of `sizes` slots (every cell its own start: `gap` unused slots behind each), probe table
    `cells` [nq, P] and list lengths `npl`"""
    rng = np.random.default_rng(seed)
    sizes = np.asarray(sizes, np.int64)
    cells = np.asarray(cells, np.int64)
    nq = cells.shape[0]
    cap = sizes + gap
    start = np.cumsum(cap) - cap
    n_slots = int(cap.sum())
    storage = rng.integers(0, 256, (16, n_slots, 4), dtype=np.uint8)
    cb = (rng.standard_normal((64, ds, 256)) * 3).astype(np.float32) if codebook is None else codebook
    q = (rng.standard_normal((64 * ds, nq)) * 3).astype(np.float32) if query is None else query
    emp = (rng.random(n_slots) < holes).astype(np.uint8)
    ok = np.clip(cells, 0, len(sizes) - 1)     # (an id out of range comes with the extents of a real cell)
    return dict(storage=storage, codebook=cb, query=q, is_empty=emp, cells=cells, npl=np.asarray(npl, np.int64),
                start=start, sizes=sizes, n_cells=len(sizes), n_slots=n_slots, cs=start[ok], sz=sizes[ok].copy(), ds=ds)


def _listed(p, first):
    """per query the live slots of its listed probes, as fetch_probes lists them"""
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


def _kernel_check(p, first, flagged=()):
    """threshold -inf: every query returns exactly its live listed slots; the `flagged` queries are flagged and
    return nothing"""
    from torchpq_amd import kernels as K
    nq = p["cells"].shape[0]
    want = _listed(p, first)
    capacity = max(64, (max(len(w) for w in want) + 63) // 64 * 64)
    assert capacity <= 4096
    count, values, address, band, flags = (t.cpu().numpy() for t in K.CellCandidatesHip()(
        _T(p["storage"]), _T(p["query"]), _T(p["codebook"]), _T(p["cells"]), p["n_cells"], _T(p["cs"]), _T(p["sz"]),
        _T(p["npl"]), torch.full((nq,), -float("inf"), device=DEV), first_probe=first, capacity=capacity,
        is_empty=_T(p["is_empty"])))
    assert sorted(np.nonzero(flags)[0].tolist()) == sorted(flagged)
    for q in range(nq):
        got = address[q, :count[q]]
        assert (address[q, count[q]:] == -1).all()
        if q in flagged:
            assert count[q] == 0
            continue
        assert count[q] == len(want[q]), (q, count[q], len(want[q]))
        assert len(set(got.tolist())) == len(got), "duplicates"
        assert set(got.tolist()) == want[q], q
    return count


def _dev(p, hint=None):
    """the problem as test_gpu_scan_cells._search takes it"""
    d = {key: _T(p[key]) for key in ("storage", "codebook", "query", "is_empty", "cells", "npl", "start", "sizes", "sz")}
    d.update(n_cells=p["n_cells"], n_slots=p["n_slots"])
    nq, P = p["cells"].shape
    # slots a query scans, on average: what the index hands over as its hint
    d["hint"] = hint or max(1, int(np.mean([np.clip(p["sz"][q, :int(np.clip(p["npl"][q], 0, P))], 0, None).sum()
                                            for q in range(nq)])))
    return d


def _rule_takes(p, d, k):
    """the host rule of the form (nq x slots_hint >= 96 n_slots among others), asked without a launch"""
    from torchpq_amd import _lib
    lib = _lib.load()
    nq, P = p["cells"].shape
    ws = lib.tpq_ivfpq_scan_workspace_bytes(nq, k, 1, 64)
    assert nq * d["hint"] >= 96 * p["n_slots"], (nq, d["hint"], p["n_slots"])
    assert lib.tpq_ivfpq_scan_route(nq, k, 1, 64, p["ds"], P, d["hint"], 0, 1, 0, 0) == 16
    assert lib.tpq_ivfpq_scan_cell_major(nq, k, 1, 64, p["ds"], P, d["hint"], 0, 1, 0, 0, p["n_cells"], p["n_slots"], ws) == 1


def _end_to_end(p, k, distance="euclidean", hint=None, **kw):
    d = _dev(p, hint)
    _rule_takes(p, d, k)
    return _check(d, k, distance, **kw)


def _perm_rows(rng, ids, nq, width):
    return np.stack([rng.permutation(ids)[:width] for _ in range(nq)])


# ---- cell counts: the prefix scan past 1 024 cells, runs of unprobed cells ------------------------------------------------
PROBED_SIZES = [33, 1, 64, 31, 65, 32, 40]


def _sparse_cells(n_cells, probed, nq, seed, ragged=True):
    rng = np.random.default_rng(seed)
    sizes = np.zeros(n_cells, np.int64)
    sizes[probed] = PROBED_SIZES[:len(probed)]
    # every query probes the probed cells in an order of its own, and two unprobed (empty) ones where there are any
    others = [c for c in (2, n_cells - 3, n_cells // 3) if 0 <= c < n_cells and c not in probed][:2]
    ids = np.array(list(probed) + others)
    cells = _perm_rows(rng, ids, nq, len(ids))
    npl = rng.integers(0, len(ids) + 1, nq) if ragged else np.full(nq, len(ids))
    npl[:3] = len(ids)
    return sizes, cells, npl


@pytest.mark.parametrize("n_cells", [1, 1023, 1024, 1025, 2049, 3000])
def test_cell_counts_at_kernel_level(n_cells):
    """cell_scan_kernel gives a thread ceil(n_cells / 1024) cells: 1, 1, 1, 2, 3, 3 here, the last threads partly or
    wholly past the end; all but a handful of cells are empty, so the binary search meets long runs of equal offsets"""
    probed = sorted({c for c in (0, 1, n_cells // 2, n_cells - 2, n_cells - 1, 1023, 1024) if 0 <= c < n_cells})
    sizes, cells, npl = _sparse_cells(n_cells, probed, 70, 100 + n_cells)
    p = _build(n_cells, sizes, cells, npl, ds=1 + n_cells % 2)
    count = _kernel_check(p, first=0 if n_cells == 1 else 1)
    assert count.max() > 0


@pytest.mark.parametrize("n_cells,probed", [(40, (5, 6, 20, 33)), (1500, (700,)), (1500, (1400, 1499)), (1500, (0, 3))])
def test_runs_of_unprobed_cells_at_kernel_level(n_cells, probed):
    """unprobed cells at the front, in the middle and at the end: equal blk_off entries under the search"""
    sizes, cells, npl = _sparse_cells(n_cells, list(probed), 70, 200 + n_cells + probed[0])
    p = _build(n_cells + probed[0], sizes, cells, npl)
    assert _kernel_check(p, first=0).max() > 0


def test_1025_cells_end_to_end():
    n_cells, nq = 1025, 1300
    probed = [0, 1, 300, 512, 700, 1000, 1023, 1024]
    rng = np.random.default_rng(31)
    sizes = np.zeros(n_cells, np.int64)
    sizes[probed] = [120, 65, 257, 33, 300, 64, 31, 255]
    p = _build(32, sizes, _perm_rows(rng, np.array(probed), nq, 8), np.full(nq, 8))
    _end_to_end(p, 10)


# ---- probe counts: the lane loops past 64 listed probes ---------------------------------------------------------------
def _many_probes(max_nprobe, nq, seed, size_hi=7, n_cells=140):
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, size_hi, n_cells)
    cells = _perm_rows(rng, np.arange(n_cells), nq, max_nprobe)
    npl = rng.integers(0, max_nprobe + 1, nq)
    npl[:8] = [0, 4, 5, 68, max_nprobe, max_nprobe, max_nprobe, 68]     # (68 > max_nprobe = 5: clamped)
    return sizes, cells, npl


@pytest.mark.parametrize("max_nprobe", [5, 68, 69, 133])
def test_probe_counts_at_kernel_level(max_nprobe):
    """first_probe = 4: 1, 64, 65 and 129 listed probes -- one, one, two and three turns of the p += 64 loops of the seed
    and scatter kernels; a cell id out of range at a probe index >= 68 flags its query when the probe is listed"""
    sizes, cells, npl = _many_probes(max_nprobe, 40, 300 + max_nprobe)
    p = _build(max_nprobe, sizes, cells, npl, ds=1 + max_nprobe % 2)
    flagged = []                           # (the id is wrong, the extents stay those of the cell it replaced)
    if max_nprobe > 68:
        p["cells"][4, 68] = len(sizes)     # listed (n_probe_list = max_nprobe): flagged
        p["cells"][7, 68] = len(sizes)     # n_probe_list = 68: never looked at
        flagged.append(4)
    if max_nprobe > 130:
        p["cells"][5, 130] = -1
        flagged.append(5)
    count = _kernel_check(p, first=4, flagged=flagged)
    assert count[0] == 0 and count[1] == 0 and count.max() > 0


def test_69_probes_end_to_end():
    nq = 1024
    sizes, cells, npl = _many_probes(69, nq, 369, size_hi=41, n_cells=72)
    p = _build(370, sizes, cells, npl)
    _end_to_end(p, 10)
    npl[9:11] = 69
    p = _build(370, sizes, cells, npl)
    p["cells"][9, 68] = len(sizes)         # (the id is wrong, the extents stay those of the cell it replaced)
    p["cells"][10, 5] = -1
    scan = _end_to_end(p, 10)
    assert scan.last_redone(nq) >= 2


# ---- repeated and void probes ---------------------------------------------------------------------------------------------
def _repeat_problem(nq, seed, sizes, **kw):
    """queries 0-3: the same cell at probes (p, p + 1), p = 2, 3, 4, 5 -- with P0 = 4 the pair lies before the boundary,
    across it and behind it; 4, 5: three times in a row (from probe 4, from probe 3); 6-8: probes of size 0 and -1, a
    void probe followed by the same cell; 9, 10: a repeated probe cut off by n_probe_list, and the only listed probe a
    repeat"""
    sizes = np.asarray(sizes)
    rng = np.random.default_rng(seed)
    n_cells, P = len(sizes), 8
    cells = _perm_rows(rng, np.arange(n_cells), nq, P)     # distinct cells per row
    npl = rng.integers(0, P + 1, nq)
    npl[:11] = P
    for q, pr in enumerate((2, 3, 4, 5)):
        cells[q, pr + 1] = cells[q, pr]
    cells[4, 5] = cells[4, 6] = cells[4, 4]
    cells[5, 4] = cells[5, 5] = cells[5, 3]
    cells[8, 5] = cells[8, 4]
    cells[9, 6] = cells[9, 5]
    npl[9] = 6
    cells[10, 4] = cells[10, 3]
    npl[10] = 5
    for q in range(11):     # overwriting a probe with its neighbour's cell keeps the row free of non-adjacent repeats
        row = cells[q]
        runs = [c for i, c in enumerate(row) if i == 0 or c != row[i - 1]]
        assert len(set(runs)) == len(runs)
    p = _build(seed + 1, sizes, cells, npl, **kw)
    p["sz"][6, 5] = 0
    p["sz"][7, 6] = -1
    p["sz"][8, 4] = 0       # void, and probe 5 lists the same cell: skipped for its start, as fetch_probes skips it
    return p


def test_repeated_and_void_probes_at_kernel_level():
    p = _repeat_problem(48, 40, [33, 40, 31, 1, 64, 65, 32, 20, 50, 7, 100, 3])
    want = _listed(p, P0)
    assert not want[10]                                    # (query 10: its only listed probe repeats probe 3)
    count = _kernel_check(p, first=P0)
    assert count[10] == 0
    # the pair across the boundary: probe 4 of query 1 is probe 3's cell again, and probe 3 is the threshold pass's
    st = p["cs"][1, 4]
    assert p["cs"][1, 3] == st and not any(st <= s < st + p["sz"][1, 4] for s in want[1])


@pytest.mark.parametrize("ds,distance,k", [(2, "euclidean", 10), (1, "inner", 100)])
def test_repeated_and_void_probes_end_to_end(ds, distance, k):
    p = _repeat_problem(1024, 41 + ds, [63, 64, 65, 255, 257, 300, 1, 120, 33, 31, 32, 90], ds=ds)
    _end_to_end(p, k, distance)


# ---- groups of queries ----------------------------------------------------------------------------------------------------
def test_cells_listed_by_1_31_32_33_64_and_65_queries():
    """a candidate block takes 32 listed queries (kCellGroup): a short group, one query short of a group, a full group,
    a group and one, two full groups, two and one"""
    nq, n_cells, n_probe = 1300, 16, 8
    p = _problem(45, nq, n_cells, n_probe, 2, ragged=False)
    g = torch.Generator(device=DEV)
    g.manual_seed(46)
    p["cells"] = torch.rand(nq, 10, generator=g, device=DEV).argsort(1)[:, :n_probe].contiguous()   # cells 0..9
    first = 0
    for cell, n in ((10, 1), (11, 31), (12, 32), (13, 33), (14, 64), (15, 65)):
        p["cells"][first:first + n, n_probe - 1] = cell
        first += n
    listed = torch.bincount(p["cells"][:, P0:].reshape(-1), minlength=n_cells)
    assert listed[10:].tolist() == [1, 31, 32, 33, 64, 65]
    assert (p["sizes"][10:] > 0).all()
    _check(p, 100)
    _check(p, 10, "inner")


# ---- tiny calls -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 3, 5])
def test_tiny_calls_at_kernel_level(nq):
    rng = np.random.default_rng(50 + nq)
    sizes = [33, 31, 65, 1, 32, 64]
    p = _build(60 + nq, sizes, _perm_rows(rng, np.arange(6), nq, 6), np.full(nq, 6), ds=1 + nq % 2)
    assert _kernel_check(p, first=1).min() > 0


@pytest.mark.parametrize("P,first", [(6, 4), (4, 4), (3, 4)])
def test_empty_listed_set_at_kernel_level(P, first):
    """every n_probe_list <= first_probe (and a probe table no wider than first_probe): counts 0, no flags"""
    rng = np.random.default_rng(70 + P)
    nq = 37
    npl = rng.integers(0, min(P, first) + 1, nq)
    npl[0] = min(P, first)
    p = _build(71 + P, [33, 31, 65, 1, 32, 64], _perm_rows(rng, np.arange(6), nq, P), npl)
    assert _kernel_check(p, first=first).max() == 0


# ---- the scale limits ---------------------------------------------------------------------------------------------------------
SCALE_SIZES = [40, 33, 64, 65, 31, 100, 120, 90]


def _magnitudes(rng, shape, top):
    """random signs, magnitudes in [1/4, 1] of `top` (a component below 2^-26 of the largest would be lost by the split;
    the caller sets one component to `top` itself)"""
    a = rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)
    return (a * top).astype(np.float32)


def _scale_problem(seed, cb_top, q_top, ds=2, nq=1024):
    rng = np.random.default_rng(seed)
    cb = _magnitudes(rng, (64, ds, 256), cb_top)
    cb[rng.integers(64), rng.integers(ds), rng.integers(256)] = cb_top
    q_top = np.broadcast_to(np.asarray(q_top, np.float64), (nq,))
    q = _magnitudes(rng, (64 * ds, nq), 1.0) * q_top[None, :].astype(np.float32)
    q[rng.integers(0, 64 * ds, nq), np.arange(nq)] = q_top
    cells = _perm_rows(rng, np.arange(8), nq, 8)
    return _build(seed + 1, SCALE_SIZES, cells, np.full(nq, 8), ds=ds, codebook=cb, query=q.astype(np.float32))


@pytest.mark.parametrize("top,ds,distance", [(2.0 ** 40 * 1.5, 2, "euclidean"), (2.0 ** -40, 2, "euclidean"),
                                             (2.0 ** 40 * 1.5, 1, "inner"), (2.0 ** -40, 1, "inner")])
def test_largest_component_at_the_scale_limit_takes_the_form(top, ds, distance):
    """2^40 x 1.5 and 2^-40 are the last binades the fp16 scaling takes: no query is handed to the exact kernel"""
    p = _scale_problem(80 + ds, top, top, ds=ds)
    scan = _end_to_end(p, 10, distance)
    assert scan.last_redone(1024) == 0


@pytest.mark.parametrize("cb_top,q_top", [(2.0 ** 41, 2.0 ** 40), (2.0 ** -41, 2.0 ** -40)])
def test_codebook_beyond_the_scale_limit_is_redone(cb_top, q_top):
    p = _scale_problem(83, cb_top, q_top)
    scan = _end_to_end(p, 10)
    assert scan.last_redone(1024) == 1024


def test_three_queries_beyond_the_scale_limit_are_redone():
    tops = np.full(1024, 2.0 ** 40 * 1.5)
    tops[[5, 500, 1023]] = 2.0 ** 41
    p = _scale_problem(84, 2.0 ** 40 * 1.5, tops)
    scan = _end_to_end(p, 10)
    assert scan.last_redone(1024) == 3


def test_degenerate_codebooks_and_subnormal_queries_are_redone():
    """an all-zero codebook and a codebook of one huge entry cannot be scaled; a query of fp32 subnormals neither"""
    p = _scale_problem(85, 1.0, 1.0)
    zero = np.zeros_like(p["codebook"])
    one = zero.copy()
    one[17, 1, 200] = 1e30
    for cb in (zero, one):
        scan = _end_to_end(dict(p, codebook=cb), 10, "inner" if cb is one else "euclidean")
        assert scan.last_redone(1024) == 1024
    rng = np.random.default_rng(86)
    mantissa = rng.integers(1, 2 ** 23, p["query"].shape).astype(np.uint32)
    sign = rng.integers(0, 2, p["query"].shape).astype(np.uint32) << 31
    sub = (mantissa | sign).view(np.float32)
    assert (np.abs(sub) < 2.0 ** -126).all() and (sub != 0).all()
    scan = _end_to_end(dict(p, query=np.ascontiguousarray(sub)), 10)
    assert scan.last_redone(1024) == 1024


# ---- a workspace used again ---------------------------------------------------------------------------------------------------
def _overflow_problem():
    """test_candidate_overflow_is_flagged_and_redone's: every query is flagged"""
    p = _problem(13, 1024, 8, 8, 2, sizes=[3, 5, 2, 7, 3000, 10, 10, 10], ragged=False)
    p["cells"] = torch.arange(8, device=DEV).repeat(1024, 1).contiguous()
    p["query"] = p["query"][:, :1].repeat(1, 1024).contiguous()
    return p


def _nan_problem():
    p = _problem(14, 1024, 8, 8, 2, ragged=False)
    p["query"][3, 7] = float("nan")
    p["query"][:, 8] = float("inf")
    p["query"][5, 9] = 1e30
    p["query"][:, 10] = 0.0
    return p


@pytest.mark.parametrize("first", ["overflow", "nan"])
def test_workspace_reuse_leaves_no_flag_behind(first):
    """one scan object, two calls of one shape: the queries flagged by the first (all of them / four) are clean in the
    second, which redoes what a fresh object redoes and equals the reference"""
    from torchpq_amd import kernels as K
    nq, k = 1024, 100
    dirty = _overflow_problem() if first == "overflow" else _nan_problem()
    scan = K.IVFPQTopkHip(m=64)
    _, scan = _search(dirty, k, scan=scan)
    assert scan.last_cell_major() is True
    assert scan.last_redone(nq) == nq if first == "overflow" else scan.last_redone(nq) >= 4
    scan.last_workspace = None     # (the allocator hands the next call of this size the same block)
    clean = _problem(15, nq, 8, 8, 2)
    got, scan = _search(clean, k, scan=scan)
    assert scan.last_cell_major() is True
    again = scan.last_redone(nq)
    fresh_out, fresh = _search(clean, k)
    ref, _ = _search(clean, k, cells=False, packed=False)
    assert again == fresh.last_redone(nq) and again < nq // 10
    for out in (got, fresh_out):
        assert torch.equal(out[0].view(torch.int32), ref[0].view(torch.int32)) and torch.equal(out[1], ref[1])
