"""GPU: the tile loop of cell_cand_kernel (csrc/scan_cells.hip) with its loads issued unconditionally a tile ahead and its
admitted rows staged in LDS, at the shapes where that loop can go wrong.

  A  tile edges and clamped loads: cells of 0, 1, 31, 32, 33, 63, 64 and 65 slots back to back in one storage whose last
     cell ends exactly at n_slots, an empty cell between two full ones, a listed cell whose extent is rejected
     (start + size > n_slots), tombstones in the first and last row of a tile; threshold -inf: per query exactly the live
     slots of its listed cells, no duplicates, nothing of a neighbouring cell (the cells touch: a row read past a size is
     a valid row of the next cell and would be admitted);
  B  staging: one cell of five tiles listed by 1, 31, 32, 33 and 64 queries at threshold -inf -- every lane admits its
     16 rows of every tile, so every tile flushes early and the block's end finds nothing left --, a finite threshold
     that admits a handful of rows per query, flushed at the block's end, and a capacity of 64 with 130 rows admitted;
  C  IVFPQIndex.search with the form on against the form off, bit for bit.

The (address, value bits) pairs are compared between the two norm paths (slot_norms True / False) in every case, and the
values against the float64 model of tests/scan_cells_oracle.py."""
import functools

import numpy as np
import pytest
import torch

import scan_cells_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(L, threshold, metric, capacity, slot_norms):
    from torchpq_amd import kernels as K
    out = K.CellCandidatesHip()(
        _T(O.storage_of(L["codes"])), _T(L["q"]), _T(L["cb"]), _T(L["cells"]), L["n_cells"], _T(L["start"][L["cells"]]),
        _T(L["sizes"][L["cells"]]), _T(L["npl"]), _T(np.asarray(threshold, np.float32)), first_probe=0,
        capacity=capacity, is_empty=_T(L["emp"]), distance=metric, slot_norms=slot_norms)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _pairs(L, out, capacity, flagged=()):
    """counts within the capacity and -1 behind the count, no duplicates -> per query (addresses ascending, value bits);
    a query in `flagged` must carry the flag and is cut at the capacity, every other must not"""
    count, values, address, band, flags = out
    got = []
    for qi in range(L["nq"]):
        assert (flags[qi] != 0) == (qi in flagged), qi
        n = min(int(count[qi]), capacity)
        assert 0 <= count[qi] and (count[qi] <= capacity or qi in flagged) and (address[qi, n:] == -1).all()
        order = np.argsort(address[qi, :n], kind="stable")
        a = address[qi, :n][order]
        assert len(np.unique(a)) == n, "duplicates"
        got.append((a, values[qi, :n][order].view(np.uint32)))
    return got


def _both(L, threshold, metric, capacity, flagged=()):
    """the two norm paths on the same inputs: identical counts, bands and (unless cut at the capacity, where the stored
    subset varies from run to run) pairs; -> pairs, band, counts"""
    with_norms = _run(L, threshold, metric, capacity, True)
    chain = _run(L, threshold, metric, capacity, False)
    a, b = _pairs(L, with_norms, capacity, flagged), _pairs(L, chain, capacity, flagged)
    assert np.array_equal(with_norms[0], chain[0])
    assert np.array_equal(with_norms[3].view(np.uint32), chain[3].view(np.uint32))
    for qi in range(L["nq"]):
        if qi in flagged:
            continue
        assert np.array_equal(a[qi][0], b[qi][0]), qi
        assert np.array_equal(a[qi][1], b[qi][1]), qi
    return a, with_norms[3], with_norms[0]


def _live(L):
    """[nq, n_slots]: the slots the kernel may admit -- listed cells whose extent lies in the storage, tombstones out"""
    live = np.zeros((L["nq"], L["n_slots"]), bool)
    for qi in range(L["nq"]):
        for c in L["cells"][qi, :L["npl"][qi]]:
            if L["start"][c] + L["sizes"][c] <= L["n_slots"]:
                live[qi, L["start"][c]:L["start"][c] + L["sizes"][c]] = True
    return live & (L["emp"][None, :] == 0)


def _check_values(got, band, r, queries):
    for qi in queries:
        a, v = got[qi][0], got[qi][1].view(np.float32).astype(np.float64)
        assert (np.abs(v - r["exact"][qi, a]) <= band[qi] / 2.0).all(), qi
        assert (np.abs(v - r["model"][qi, a]) <= r["tol"][qi, a]).all(), qi


# ---- A ---------------------------------------------------------------------------------------------------------------
# a full cell, the empty one, a full one; then the other sizes; cell 8 is listed with an extent that leaves the storage
A_SIZES = np.array([32, 0, 64, 1, 31, 33, 63, 65, 20])
A_START = np.concatenate([np.cumsum(A_SIZES[:8]) - A_SIZES[:8], [289 - 10]])
A_START[1] = 289    # (a probe whose start repeats the previous probe's is skipped as a repeat: the empty cell gets its own)
A_CAPACITY = 320


@functools.lru_cache(maxsize=None)
def _layout_a(ds):
    nq, n_cells = 40, len(A_SIZES)               # 40 queries: a full group of 32 and a short one per cell
    n_slots = int(A_SIZES[:8].sum())
    assert n_slots == 289 == A_START[7] + A_SIZES[7] and A_START[8] + A_SIZES[8] > n_slots
    cb, q, codes = O.family("random", ds, nq, n_slots, seed=11)
    rng = np.random.default_rng([13, ds])
    emp = np.zeros(n_slots, np.uint8)
    # tombstones in the first and last row of a tile: both rows of the 32-slot cell, the full tiles of the 64-, 63- and
    # 65-slot cells, the one-row last tiles of the 33- and 65-slot cells, the ragged last rows of the 31- and 63-slot
    # ones; the one-slot cell stays live
    for cell, rows in ((0, (0, 31)), (2, (0, 31, 32, 63)), (4, (0, 30)), (5, (31, 32)), (6, (0, 31, 32, 62)),
                       (7, (0, 31, 32, 63, 64))):
        emp[A_START[cell] + np.array(rows)] = 1
    cells = np.stack([rng.permutation(n_cells) for _ in range(nq)]).astype(np.int64)
    npl = rng.integers(1, n_cells + 1, nq).astype(np.int64)
    npl[:6] = [0, 1, 2, n_cells, n_cells, n_cells]
    return dict(cb=cb, q=q, codes=codes, emp=emp, cells=cells, npl=npl, start=A_START, sizes=A_SIZES, nq=nq,
                n_cells=n_cells, n_slots=n_slots)


@functools.lru_cache(maxsize=None)
def _reference_a(ds, metric):
    L = _layout_a(ds)
    return O.evaluate(L["q"], L["cb"], L["codes"], metric)


@pytest.mark.parametrize("metric", O.METRICS)
@pytest.mark.parametrize("ds", [1, 2])
def test_tile_edges_and_clamped_loads(ds, metric):
    L = _layout_a(ds)
    live = _live(L)
    assert live.sum(1).max() <= A_CAPACITY and live.sum(1).max() == (L["emp"] == 0).sum()
    got, band, count = _both(L, np.full(L["nq"], -np.inf), metric, A_CAPACITY)
    for qi in range(L["nq"]):
        assert np.array_equal(got[qi][0], np.nonzero(live[qi])[0]), qi
    assert np.array_equal(count, live.sum(1))
    _check_values(got, band, _reference_a(ds, metric), range(L["nq"]))


# ---- B ---------------------------------------------------------------------------------------------------------------
B_LISTED = [1, 31, 32, 33, 64]
B_SIZE, B_START = 130, 3                        # five tiles, the last of two rows
B_CAPACITY = 192


@functools.lru_cache(maxsize=None)
def _reference_b(ds, metric):
    """64 queries over the cell, evaluated once; a case takes the first n of them"""
    n_slots = B_START + B_SIZE
    cb, q, codes = O.family("random", ds, max(B_LISTED), n_slots, seed=17)
    return cb, q, codes, O.evaluate(q, cb, codes, metric)


def _layout_b(n, ds, metric):
    cb, q, codes, r = _reference_b(ds, metric)
    n_slots = B_START + B_SIZE
    L = dict(cb=cb, q=np.ascontiguousarray(q[:, :n]), codes=codes, emp=np.zeros(n_slots, np.uint8),
             cells=np.zeros((n, 1), np.int64), npl=np.ones(n, np.int64), start=np.array([B_START]),
             sizes=np.array([B_SIZE]), nq=n, n_cells=1, n_slots=n_slots)
    return L, r


@pytest.mark.parametrize("ds,metric", [(2, "euclidean"), (1, "inner")])
@pytest.mark.parametrize("n", B_LISTED)
def test_every_tile_overflows_the_segments(n, ds, metric):
    L, r = _layout_b(n, ds, metric)
    got, band, count = _both(L, np.full(n, -np.inf), metric, B_CAPACITY)
    assert count.sum() == B_SIZE * n and (count == B_SIZE).all()
    for qi in range(n):
        assert np.array_equal(got[qi][0], np.arange(B_START, B_START + B_SIZE)), qi
    _check_values(got, band, r, range(n))


@pytest.mark.parametrize("ds,metric", [(2, "euclidean"), (1, "inner")])
def test_a_handful_of_rows_waits_for_the_end_of_the_block(ds, metric):
    n = 33
    L, r = _layout_b(n, ds, metric)
    every, band, _ = _both(L, np.full(n, -np.inf), metric, B_CAPACITY)
    # tau: the query's 4th largest value.  The kernel admits v >= fl(tau - delta_q) with band = 2 delta_q, and v has the
    # bits of the first call: the admitted set is known exactly
    tau = np.array([np.sort(g[1].view(np.float32))[-4] for g in every], np.float32)
    got, band2, count = _both(L, tau, metric, B_CAPACITY)
    assert np.array_equal(band.view(np.uint32), band2.view(np.uint32))
    admit = (tau - band / np.float32(2)).astype(np.float32)
    for qi in range(n):
        a, v = every[qi][0], every[qi][1].view(np.float32)
        keep = v >= admit[qi]
        assert 4 <= keep.sum() == count[qi] < B_SIZE // 2, qi
        assert np.array_equal(got[qi][0], a[keep]) and np.array_equal(got[qi][1], every[qi][1][keep]), qi


@pytest.mark.parametrize("ds,metric", [(2, "euclidean"), (1, "inner")])
def test_capacity_64_with_130_rows_admitted(ds, metric):
    n, over = 8, (0, 5)
    L, r = _layout_b(n, ds, metric)
    every, band, _ = _both(L, np.full(n, -np.inf), metric, B_CAPACITY)
    tau = np.array([np.sort(g[1].view(np.float32))[-4] for g in every], np.float32)
    tau[list(over)] = -np.inf
    got, band2, count = _both(L, tau, metric, 64, flagged=over)
    admit = (tau - band / np.float32(2)).astype(np.float32)
    for qi in range(n):
        a, v = every[qi][0], every[qi][1].view(np.float32)
        if qi in over:
            # flagged (checked in _pairs), every admitted row counted, 64 distinct slots of the cell stored with their values
            assert count[qi] == B_SIZE and len(got[qi][0]) == 64
            assert np.isin(got[qi][0], a).all()
            assert np.array_equal(got[qi][1], every[qi][1][np.searchsorted(a, got[qi][0])]), qi
            continue
        keep = v >= admit[qi]
        assert 4 <= keep.sum() == count[qi] <= 64, qi
        assert np.array_equal(got[qi][0], a[keep]) and np.array_equal(got[qi][1], every[qi][1][keep]), qi


# ---- C ---------------------------------------------------------------------------------------------------------------
def test_whole_route_against_the_form_switched_off():
    from torchpq_amd.index import IVFPQIndex
    rng = np.random.default_rng(23)
    d, n, nq, n_cells, n_probe = 64, 8192, 1024, 32, 12   # 1 024 queries x 12 / 32 of the slots: 384 re-reads (>= 96)
    centers = rng.standard_normal((d, n_cells)) * 4
    base = (centers[:, rng.integers(0, n_cells, n)] + rng.standard_normal((d, n))).astype(np.float32)
    np.random.seed(23)
    idx = IVFPQIndex(d_vector=d, n_subvectors=64, n_cells=n_cells, initial_size=1024, device=DEV, verbose=0)
    x = torch.from_numpy(base).to(DEV)
    idx.train(x)
    ids = idx.add(x)
    idx.remove(ids=ids[::9].contiguous())
    idx.n_probe = n_probe
    idx.use_smart_probing = False
    xq = (x[:, :nq] + 0.05).contiguous()
    scan = idx._ivfpq_topk._scan
    for k in (10, 100):
        idx.use_cell_major = True
        v, i = idx.search(xq, k=k)
        assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is True
        idx.use_cell_major = False
        v0, i0 = idx.search(xq, k=k)
        assert scan.last_cell_major() is False
        torch.cuda.synchronize()
        assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(i, i0)
    idx.use_cell_major = True
