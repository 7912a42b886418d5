"""GPU: the tile epilogue of cell_cand_kernel (csrc/scan_cells.hip) -- the one-fma admission test against the folded
threshold, the rows staged under their compare's mask, the flush in front of a row that does not fit -- through
CellCandidatesHip, both metrics, ds = 1 and 2, the workspace with and without room for the slot norms.

  ties       one call at threshold -inf returns every live slot's key.  A second call sets each query's threshold so that
             fl(thr - delta_q) is exactly one of those keys: that slot is admitted, and the admitted set is the set
             computed on the host from the first call's keys; a third call, with the next float up, does not admit it;
  placement  32 one-query cells of 33 slots; in cell p only slot p -- the query itself -- can pass: the address returned
             is start + p (the row <-> accumulator register mapping in both half-waves, and the one-row second tile);
  edges      cells of 1, 31, 32, 33, 64 and 65 slots back to back, the last row of each a tombstone that would pass,
             listed by groups of 1, 31, 32 and 33 queries at threshold -inf;
  staging    a cell of 300 slots at threshold -inf: every lane overruns its seven entries in the middle of a tile, twice
             per tile, ten tiles long; and queries whose candidates overflow the capacity between queries that do not."""
import functools

import numpy as np
import pytest
import torch

import scan_cells_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = [(ds, metric, norms) for ds in (1, 2) for metric in O.METRICS for norms in (True, False)]
IDS = ["ds%d-%s-%s" % (ds, metric, "norms" if norms else "chain") for ds, metric, norms in CASES]
cases = pytest.mark.parametrize("ds,metric,norms", CASES, ids=IDS)


def _T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _run(L, threshold, metric, capacity, norms):
    from torchpq_amd import kernels as K
    out = K.CellCandidatesHip()(
        _T(O.storage_of(L["codes"])), _T(L["q"]), _T(L["cb"]), _T(L["cells"]), L["n_cells"], _T(L["start"][L["cells"]]),
        _T(L["sizes"][L["cells"]]), _T(L["npl"]), _T(np.asarray(threshold, np.float32)), first_probe=0,
        capacity=capacity, is_empty=_T(L["emp"]), distance=metric, slot_norms=norms)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in out]


def _pairs(L, out, capacity, flagged=()):
    """-> per query (addresses ascending, values); counts within the capacity, -1 behind the count, no duplicates, the
    flag on exactly the queries in `flagged`"""
    count, values, address, band, flags = out
    got = []
    for qi in range(L["nq"]):
        assert (flags[qi] != 0) == (qi in flagged), qi
        n = min(int(count[qi]), capacity)
        assert 0 <= count[qi] and (count[qi] <= capacity or qi in flagged) and (address[qi, n:] == -1).all(), qi
        order = np.argsort(address[qi, :n], kind="stable")
        a = address[qi, :n][order]
        assert len(np.unique(a)) == n, "duplicates"
        got.append((a, values[qi, :n][order]))
    return got


def _layout(cb, q, codes, sizes, cells, npl, emp=None):
    sizes = np.asarray(sizes, np.int64)
    start = np.cumsum(sizes) - sizes
    n_slots = int(sizes.sum())
    assert codes.shape[0] == n_slots
    return dict(cb=cb, q=q, codes=codes, emp=np.zeros(n_slots, np.uint8) if emp is None else emp,
                cells=np.asarray(cells, np.int64), npl=np.asarray(npl, np.int64), start=start, sizes=sizes,
                nq=q.shape[1], n_cells=len(sizes), n_slots=n_slots)


def _live(L):
    live = np.zeros((L["nq"], L["n_slots"]), bool)
    for qi in range(L["nq"]):
        for c in L["cells"][qi, :L["npl"][qi]]:
            live[qi, L["start"][c]:L["start"][c] + L["sizes"][c]] = True
    return live & (L["emp"][None, :] == 0)


def _up(v):
    return np.nextafter(np.float32(v), np.float32(np.inf))


# ---- ties ------------------------------------------------------------------------------------------------------------
T_SIZES = [70, 33, 40]
T_NQ = 40                                       # a full group of 32 and a short one per cell
T_CAPACITY = 192


@functools.lru_cache(maxsize=None)
def _layout_ties(ds):
    cb, q, codes = O.family("random", ds, T_NQ, sum(T_SIZES), seed=41)
    emp = np.zeros(sum(T_SIZES), np.uint8)
    emp[[0, 69, 70, 110]] = 1
    return _layout(cb, q, codes, T_SIZES, np.tile(np.arange(3), (T_NQ, 1)), np.full(T_NQ, 3), emp)


def _tau_for(target, delta):
    """a float32 tau with fl(tau - delta) == target, or None"""
    t0 = np.float32(target + delta)
    for step in range(-4, 5):
        tau = t0
        for _ in range(abs(step)):
            tau = np.nextafter(tau, np.float32(np.inf if step > 0 else -np.inf))
        if np.float32(tau - delta) == target:
            return tau
    return None


@cases
def test_threshold_ties(ds, metric, norms):
    L = _layout_ties(ds)
    nq = L["nq"]
    first = _run(L, np.full(nq, -np.inf), metric, T_CAPACITY, norms)
    every = _pairs(L, first, T_CAPACITY)
    live = _live(L)
    for qi in range(nq):
        assert np.array_equal(every[qi][0], np.nonzero(live[qi])[0]), qi
    delta = (first[3] / np.float32(2)).astype(np.float32)             # band = 2 delta_q, a power-of-two factor: exact
    # per query a key of the first call, from the middle of its sorted keys, that fl(tau - delta_q) can hit exactly and
    # whose upper neighbour it can hit as well
    tau_at, tau_above, target = np.zeros(nq, np.float32), np.zeros(nq, np.float32), np.zeros(nq, np.float32)
    for qi in range(nq):
        vs = np.sort(every[qi][1])
        for v in vs[len(vs) // 2:]:
            a, b = _tau_for(v, delta[qi]), _tau_for(_up(v), delta[qi])
            if a is not None and b is not None:
                tau_at[qi], tau_above[qi], target[qi] = a, b, v
                break
        else:
            raise AssertionError("no key of query %d can be hit exactly" % qi)
    for tau, admit in ((tau_at, target), (tau_above, _up(target))):
        out = _run(L, tau, metric, T_CAPACITY, norms)
        assert np.array_equal(out[3].view(np.uint32), first[3].view(np.uint32))
        assert np.array_equal((tau - delta).astype(np.float32), admit)
        got = _pairs(L, out, T_CAPACITY)
        for qi in range(nq):
            a, v = every[qi]
            keep = v >= admit[qi]
            assert np.array_equal(got[qi][0], a[keep]), qi             # equal as sets: both ascending, no duplicates
            assert np.array_equal(got[qi][1].view(np.uint32), v[keep].view(np.uint32)), qi
            assert out[0][qi] == keep.sum()
            tied = a[v == target[qi]]
            assert len(tied) >= 1 and np.isin(tied, got[qi][0]).all() == (admit is target), qi


# ---- placement -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layout_placement(ds):
    n_cells, size = 32, 33
    cb, _, codes = O.family("random", ds, 1, n_cells * size, seed=43)
    x = O.decode(cb, codes)
    q = np.ascontiguousarray(x[np.arange(n_cells) * size + np.arange(n_cells)].T)    # query p = slot p of cell p
    return _layout(cb, q, codes, [size] * n_cells, np.arange(n_cells)[:, None], np.ones(n_cells)), x


@cases
def test_row_placement(ds, metric, norms):
    L, x = _layout_placement(ds)
    ex = O.exact(L["q"].T, x, metric)
    tau, margin = np.zeros(32, np.float32), np.zeros(32)
    for p in range(32):
        mine = ex[p, 33 * p:33 * p + 33]
        tau[p] = (mine[p] + np.delete(mine, p).max()) / 2
        margin[p] = mine[p] - np.delete(mine, p).max()
    out = _run(L, tau, metric, 64, norms)
    assert (margin > 8 * out[3]).all()                                 # (slot p stands out by far more than the band)
    got = _pairs(L, out, 64)
    for p in range(32):
        assert np.array_equal(got[p][0], [33 * p + p]), p


# ---- edges -----------------------------------------------------------------------------------------------------------
E_SIZES = [1, 31, 32, 33, 64, 65]
E_CAPACITY = 256


@functools.lru_cache(maxsize=None)
def _data_edges(ds):
    return O.family("random", ds, 33, sum(E_SIZES), seed=47)


@pytest.mark.parametrize("n", [1, 31, 32, 33])
@cases
def test_tile_edges_with_a_tombstone_in_the_last_row(ds, metric, norms, n):
    cb, q, codes = _data_edges(ds)
    emp = np.zeros(sum(E_SIZES), np.uint8)
    emp[np.cumsum(E_SIZES) - 1] = 1
    L = _layout(cb, np.ascontiguousarray(q[:, :n]), codes, E_SIZES, np.tile(np.arange(6), (n, 1)), np.full(n, 6), emp)
    out = _run(L, np.full(n, -np.inf), metric, E_CAPACITY, norms)
    got = _pairs(L, out, E_CAPACITY)
    expect = np.nonzero(emp == 0)[0]
    for qi in range(n):
        assert np.array_equal(got[qi][0], expect), qi
    assert (out[0] == len(expect)).all()


# ---- staging ---------------------------------------------------------------------------------------------------------
S_SIZE, S_NQ = 300, 33


@functools.lru_cache(maxsize=None)
def _reference_staging(ds, metric):
    cb, q, codes = O.family("random", ds, S_NQ, S_SIZE, seed=53)
    return cb, q, codes, O.evaluate(q, cb, codes, metric)


@functools.lru_cache(maxsize=None)
def _every_staging(ds, metric, norms):
    """the cell at threshold -inf with room for everything: checked, then the reference of the overflow case"""
    cb, q, codes, r = _reference_staging(ds, metric)
    L = _layout(cb, q, codes, [S_SIZE], np.zeros((S_NQ, 1)), np.ones(S_NQ))
    out = _run(L, np.full(S_NQ, -np.inf), metric, 320, norms)
    return L, r, out, _pairs(L, out, 320)


@cases
def test_every_lane_overruns_its_segment_mid_tile(ds, metric, norms):
    L, r, out, got = _every_staging(ds, metric, norms)
    assert (out[0] == S_SIZE).all()
    for qi in range(S_NQ):
        a, v = got[qi][0], got[qi][1].astype(np.float64)
        assert np.array_equal(a, np.arange(S_SIZE)), qi
        assert (np.abs(v - r["exact"][qi]) <= out[3][qi] / 2.0).all(), qi
        assert (np.abs(v - r["model"][qi]) <= r["tol"][qi]).all(), qi
    if not norms:                                                      # the two norm paths: the same keys
        other = _every_staging(ds, metric, True)[3]
        for qi in range(S_NQ):
            assert np.array_equal(got[qi][1].view(np.uint32), other[qi][1].view(np.uint32)), qi


@cases
def test_overflowing_queries_between_queries_that_fit(ds, metric, norms):
    L, r, first, every = _every_staging(ds, metric, norms)
    over = (3, 17, 31)
    delta = (first[3] / np.float32(2)).astype(np.float32)
    tau = np.array([np.sort(g[1])[-20] for g in every], np.float32)   # 20 or so rows each ...
    tau[list(over)] = -np.inf                                          # ... and all 300 into 64 entries
    out = _run(L, tau, metric, 64, norms)
    got = _pairs(L, out, 64, flagged=over)
    admit = (tau - delta).astype(np.float32)
    for qi in range(S_NQ):
        a, v = every[qi]
        if qi in over:
            assert out[0][qi] == S_SIZE and len(got[qi][0]) == 64
            assert np.array_equal(got[qi][1].view(np.uint32), v[got[qi][0]].view(np.uint32)), qi
            continue
        keep = v >= admit[qi]
        assert 20 <= keep.sum() == out[0][qi] <= 64, qi
        assert np.array_equal(got[qi][0], a[keep]), qi
        assert np.array_equal(got[qi][1].view(np.uint32), v[keep].view(np.uint32)), qi
