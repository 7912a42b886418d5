"""GPU: the per-call slot norms of the cell-major form (cell_norm_kernel and cell_cand_kernel<DS, true>,
csrc/scan_cells.hip) against the candidate kernel's own chain (cell_cand_kernel<DS, false>): the norm array holds the bits
the chain forms, so the two paths admit the same slots with the same keys.

  A  CellCandidatesHip with slot_norms=True against False: per query the (address, value bits) pairs are identical and
     are the live slots of the listed cells (threshold -inf), and at a finite threshold identical again and exactly the
     slots whose value reaches it;
  B  one cell listed by 1 ... 129 queries (the edges of the 32-column groups of a block), a second cell by one query,
     thresholds -inf and +large alternating: nothing of one query under another, values against the float64 model of
     tests/scan_cells_oracle.py;
  C  IVFPQIndex.search with the default workspace (norms), with exactly lists + extras (no norms) and with the form off:
     values and ids bit-equal three ways, again after a remove and an add (the norms are per call)."""
import functools

import numpy as np
import pytest
import torch

import scan_cells_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(L, threshold, metric, first, capacity, slot_norms):
    from torchpq_amd import kernels as K
    out = K.CellCandidatesHip()(
        _T(O.storage_of(L["codes"])), _T(L["q"]), _T(L["cb"]), _T(L["cells"]), L["n_cells"], _T(L["start"][L["cells"]]),
        _T(L["sizes"][L["cells"]]), _T(L["npl"]), _T(np.asarray(threshold, np.float32)), first_probe=first,
        capacity=capacity, is_empty=_T(L["emp"]), distance=metric, slot_norms=slot_norms)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _pairs(L, out, capacity):
    """flags 0, counts within the capacity, -1 behind the count -> per query (addresses ascending, value bits)"""
    count, values, address, band, flags = out
    assert not flags.any(), "a flagged query: the comparison would be empty"
    got = []
    for qi in range(L["nq"]):
        n = count[qi]
        assert 0 <= n <= capacity and (address[qi, n:] == -1).all()
        order = np.argsort(address[qi, :n], kind="stable")
        a = address[qi, :n][order]
        assert len(np.unique(a)) == n, "duplicates"
        got.append((a, values[qi, :n][order].view(np.uint32)))
    return got


def _both(L, threshold, metric, first, capacity):
    """the two kernels on the same inputs: identical pairs, bands and counts; -> pairs, values' band"""
    with_norms = _run(L, threshold, metric, first, capacity, True)
    chain = _run(L, threshold, metric, first, capacity, False)
    a, b = _pairs(L, with_norms, capacity), _pairs(L, chain, capacity)
    assert np.array_equal(with_norms[0], chain[0]) and np.array_equal(with_norms[3].view(np.uint32), chain[3].view(np.uint32))
    for qi in range(L["nq"]):
        assert np.array_equal(a[qi][0], b[qi][0]), qi
        assert np.array_equal(a[qi][1], b[qi][1]), qi
    return a, with_norms[3]


def _live(L, first):
    live = np.zeros((L["nq"], L["n_slots"]), bool)
    for qi in range(L["nq"]):
        for c in L["cells"][qi, first:L["npl"][qi]]:
            live[qi, L["start"][c]:L["start"][c] + L["sizes"][c]] = True
    return live & (L["emp"][None, :] == 0)


# ---- A ---------------------------------------------------------------------------------------------------------------
A_SIZES = np.array([0, 1, 31, 33, 64, 977])
A_START = np.array([1, 3, 6, 39, 75, 141])      # no start is a multiple of 4; cells do not touch
A_CAPACITY = 1152                               # >= 1 + 31 + 33 + 64 + 977


@functools.lru_cache(maxsize=None)
def _layout_a(ds):
    nq, n_cells = 40, len(A_SIZES)               # 40 queries: a full group of 32 and a short one per cell
    assert (A_START % 4 != 0).all() and (A_START[1:] >= A_START[:-1] + A_SIZES[:-1]).all()
    n_slots = int(A_START[-1] + A_SIZES[-1] + 3)
    cb, q, codes = O.family("random", ds, nq, n_slots, seed=5)
    rng = np.random.default_rng([7, ds])
    emp = (rng.random(n_slots) < 0.03).astype(np.uint8)
    emp[A_START[1]] = 0                          # the one-slot cell stays live
    # tombstones in the first, a middle and the last row of a tile: the first and the last (ragged, 17 rows) tile of
    # the large cell, both tiles of the 64-slot cell, the one-row second tile of the 33-slot cell
    for cell, rows in ((5, (0, 15, 31, 960, 968, 976)), (4, (0, 31, 32, 47, 63)), (3, (32,)), (2, (0, 30))):
        emp[A_START[cell] + np.array(rows)] = 1
    cells = np.stack([rng.permutation(n_cells) for _ in range(nq)]).astype(np.int64)
    npl = rng.integers(0, n_cells + 1, nq).astype(np.int64)
    npl[:6] = [0, 1, 2, 3, n_cells, n_cells]
    return dict(cb=cb, q=q, codes=codes, emp=emp, cells=cells, npl=npl, start=A_START, sizes=A_SIZES, nq=nq,
                n_cells=n_cells, n_slots=n_slots)


@pytest.mark.parametrize("first", [0, 2])
@pytest.mark.parametrize("metric", O.METRICS)
@pytest.mark.parametrize("ds", [1, 2])
def test_norms_against_the_chain(ds, metric, first):
    L = _layout_a(ds)
    nq = L["nq"]
    live = _live(L, first)
    assert live.sum(1).max() <= A_CAPACITY
    got, band = _both(L, np.full(nq, -np.inf), metric, first, A_CAPACITY)
    for qi in range(nq):
        assert np.array_equal(got[qi][0], np.nonzero(live[qi])[0]), qi
    # a finite threshold: the median of the values the query was just given.  The kernel admits v >= fl(tau - delta_q)
    # with band = 2 delta_q, and v has the bits of the first call: the admitted set is known exactly
    tau = np.array([np.median(g[1].view(np.float32)) if len(g[1]) else 0.0 for g in got], np.float32)
    again, band2 = _both(L, tau, metric, first, A_CAPACITY)
    assert np.array_equal(band.view(np.uint32), band2.view(np.uint32))
    admit = (tau - band / np.float32(2)).astype(np.float32)
    some = 0
    for qi in range(nq):
        a, v = got[qi][0], got[qi][1].view(np.float32)
        keep = v >= admit[qi]
        assert np.array_equal(again[qi][0], a[keep]) and np.array_equal(again[qi][1], got[qi][1][keep]), qi
        some += int(0 < keep.sum() < len(keep))
    assert some >= nq // 5, "the finite threshold cuts nothing"   # (queries that list nothing or one slot have no cut)


# ---- B ---------------------------------------------------------------------------------------------------------------
B_LISTED = [1, 31, 32, 33, 63, 64, 65, 96, 97, 129]
B_SIZES = np.array([70, 33])                    # three tiles, the last of 6 rows; two tiles, the last of one row
B_START = np.array([2, 75])
B_CAPACITY = 128


@functools.lru_cache(maxsize=None)
def _reference_b(ds, metric):
    """130 queries over the two cells, evaluated once; a case takes the first n + 1 of them"""
    n_slots = int(B_START[-1] + B_SIZES[-1] + 1)
    cb, q, codes = O.family("random", ds, max(B_LISTED) + 1, n_slots, seed=9)
    emp = np.zeros(n_slots, np.uint8)
    emp[B_START[0] + np.array([0, 31, 40, 69])] = 1
    emp[B_START[1] + 32] = 1
    return cb, q, codes, emp, O.evaluate(q, cb, codes, metric)


@pytest.mark.parametrize("ds,metric", [(2, "euclidean"), (1, "inner")])
@pytest.mark.parametrize("n", B_LISTED)
def test_groups_of_a_block(n, ds, metric):
    cb, q, codes, emp, r = _reference_b(ds, metric)
    nq = n + 1
    cells = np.zeros((nq, 1), np.int64)
    cells[n, 0] = 1                              # the last query lists the second cell, alone
    L = dict(cb=cb, q=np.ascontiguousarray(q[:, :nq]), codes=codes, emp=emp, cells=cells, npl=np.ones(nq, np.int64),
             start=B_START, sizes=B_SIZES, nq=nq, n_cells=2, n_slots=len(emp))
    live = _live(L, 0)
    # distinct thresholds per query: every other query admits everything, the others nothing
    tau = np.where(np.arange(nq) % 2 == 0, -np.inf, 1e30).astype(np.float32)
    tau[n] = -np.inf
    got, band = _both(L, tau, metric, 0, B_CAPACITY)
    B = O.bound_B(L["q"], cb)
    assert (band.astype(np.float64) / 2 >= O.delta_rel(ds) * B * B).all()
    for qi in range(nq):
        a, v = got[qi][0], got[qi][1].view(np.float32).astype(np.float64)
        if tau[qi] > 0:
            assert len(a) == 0, qi
            continue
        assert np.array_equal(a, np.nonzero(live[qi])[0]), qi
        assert (np.abs(v - r["exact"][qi, a]) <= band[qi] / 2.0).all(), qi
        assert (np.abs(v - r["model"][qi, a]) <= r["tol"][qi, a]).all(), qi


# ---- C ---------------------------------------------------------------------------------------------------------------
def _align(n):
    return (n + 255) // 256 * 256


def test_whole_route_three_ways_and_after_an_update():
    from torchpq_amd import _lib
    from torchpq_amd.index import IVFPQIndex
    lib = _lib.load()
    rng = np.random.default_rng(21)
    d, n, nq, n_cells, n_probe = 64, 4000, 1024, 8, 8
    centers = rng.standard_normal((d, n_cells)) * 4
    base = (centers[:, rng.integers(0, n_cells, n + 600)] + rng.standard_normal((d, n + 600))).astype(np.float32)
    np.random.seed(21)
    idx = IVFPQIndex(d_vector=d, n_subvectors=64, n_cells=n_cells, initial_size=1024, device=DEV, verbose=0)
    x = torch.from_numpy(base).to(DEV)
    idx.train(x[:, :n].contiguous())
    ids = idx.add(x[:, :n].contiguous())
    idx.n_probe = n_probe
    idx.use_smart_probing = False
    xq = (x[:, :nq] + 0.05).contiguous()
    scan = idx._ivfpq_topk._scan
    lists16 = 2 * _align(nq * 4) + nq * 16 * 64 * 8 + _align(nq * 16 * 4)
    no_room = lists16 + lib.tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, n_cells, 4)

    def three_ways(k):
        scan.workspace_bytes, idx.use_cell_major = None, True
        v, i = idx.search(xq, k=k)
        assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is True and scan.last_cell_norms() is True
        scan.workspace_bytes = no_room
        v1, i1 = idx.search(xq, k=k)
        assert scan.last_cell_major() is True and scan.last_cell_norms() is False
        scan.workspace_bytes, idx.use_cell_major = None, False
        v0, i0 = idx.search(xq, k=k)
        assert scan.last_cell_major() is False and scan.last_cell_norms() is False
        idx.use_cell_major = True
        torch.cuda.synchronize()
        for vv, ii in ((v1, i1), (v0, i0)):
            assert torch.equal(v.view(torch.int32), vv.view(torch.int32)) and torch.equal(i, ii)
        return v, i

    before = {k: three_ways(k) for k in (10, 100)}
    # the norms are per call: tombstones and new codes in the same slots must show in the next call
    idx.remove(ids=ids[::7].contiguous())
    idx.add(x[:, n:].contiguous())
    for k in (10, 100):
        v, i = three_ways(k)
        assert not torch.equal(i, before[k][1])
        assert not torch.isin(i, ids[::7]).any()
