"""GPU: the threshold form of the cell-major scan (csrc/scan_cells.hip, `The threshold from group maxima`: pass A's group
maxima over the first T probes, cell_kth_kernel, the candidates of all probes, the finish kernel without seed chunks)
against the reference-layout kernel (`packed=None`), values bit for bit and addresses entry for entry; two replays of
a captured search against the eager call; the form under guarded, pre-filled allocations; and the first pass, read back
from the kept workspace, against float64 numpy.
Cells are 512 ... 1 100 slots long: the form is taken from a mean probed cell of 512 slots on."""
import numpy as np
import pytest
import torch

from test_gpu_scan_cells import DEV, _problem, _search
from test_scan_cell_maxima_cpu import G, T

pytestmark = pytest.mark.gpu

# (1 025 slots with 5 % tombstones, or a ragged list of one such cell, still fit the 1 024 entries of a query's lists)
SIZES = [512, 513, 543, 544, 545, 1025, 700, 900]
# the same edge sizes at a mean of 708 slots: T x mean / G >= 2 k holds for k = 128 at T = 6, G = 16 (265 >= 256)
SIZES_LONG = [600, 513, 543, 544, 545, 1025, 900, 1000]


def _gate(p, k):
    """what the library's rule says for the call _search makes of p (host arithmetic, restated)"""
    n_probe = p["cells"].shape[1]
    hint = p.get("hint") or int(p["sizes"].float().mean().item() * n_probe)
    mean = hint // n_probe
    return n_probe > T and mean >= 512 and T * mean // G >= 2 * k and k <= 128


def _big(seed, nq, n_probe, ds, sizes=None, k=1, **kw):
    n_cells = 8 if n_probe <= 8 else 16
    sizes = sizes or (SIZES_LONG if k > 100 else SIZES) * (n_cells // 8)
    p = _problem(seed, nq, n_cells, n_probe, ds, sizes=sizes, **kw)
    if kw.get("ragged", True):
        p["npl"][:8] = torch.tensor([0, 1, T - 1, T, T + 1, n_probe, 2, n_probe], device=DEV)
    return p


def _check(p, k, distance="euclidean", nan_rows=None, expect=None):
    got, scan = _search(p, k, distance)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is True
    expect = _gate(p, k) if expect is None else expect
    assert scan.last_cell_threshold() is expect
    ref, _ = _search(p, k, distance, cells=False, packed=False)
    ok = torch.ones(got[0].shape[0], dtype=torch.bool, device=DEV)
    if nan_rows is not None:
        ok[nan_rows] = False
    assert torch.equal(got[0][ok].view(torch.int32), ref[0][ok].view(torch.int32))
    assert torch.equal(got[1], ref[1])
    return scan


CASES = [  # nq, n_probe, ds, distance, k
    (1024, T + 1, 2, "euclidean", 100), (1024, 12, 1, "inner", 10), (1024, T + 1, 1, "euclidean", 1),
    (1024, 12, 2, "inner", 128), (1025, T + 1, 1, "inner", 128), (1025, 12, 2, "euclidean", 10),
    (1025, T + 1, 2, "inner", 100), (1025, 12, 1, "euclidean", 100), (1300, T + 1, 2, "euclidean", 1),
    (1300, 12, 1, "euclidean", 128), (1300, T + 1, 1, "inner", 10), (1300, 12, 2, "euclidean", 100),
]


@pytest.mark.parametrize("nq,n_probe,ds,distance,k", CASES)
def test_equals_the_reference_layout_kernel(nq, n_probe, ds, distance, k):
    """cells of 512, 513, 543, 544, 545, 700, 900 and 1 025 slots (k = 128: 513 ... 1 025 at a mean of 708, so that the
    rule takes the form there too), 5 % tombstones, every query with all its probes.  Every case runs the form"""
    p = _big(nq + n_probe + k, nq, n_probe, ds, k=k, ragged=False)
    assert _gate(p, k)
    scan = _check(p, k, distance, expect=True)
    assert scan.last_redone(nq) == 0


@pytest.mark.parametrize("n_probe,ds,distance,k", [(T + 1, 2, "euclidean", 100), (12, 1, "inner", 10),
                                                   (12, 2, "euclidean", 128)])
def test_ragged_probe_counts(n_probe, ds, distance, k):
    """probe counts drawn from 0 ... n_probe, and 0, 1, T - 1, T, T + 1 among them: queries with nothing behind the first
    pass, queries with fewer than k maxima (threshold -inf: everything is admitted; two cells of 900 and 545 slots are
    94 maxima at G = 16 and 1 373 live slots, more than the lists hold, so such a query is flagged and redone exactly).
    Only queries whose first pass reserves fewer than k maxima may be redone"""
    p = _big(31 + n_probe + k, 1300, n_probe, ds, k=k, ragged=True)
    assert _gate(p, k)
    scan = _check(p, k, distance, expect=True)
    tiles = (p["sizes"][p["cells"]] + 31) // 32
    listed = torch.arange(n_probe, device=DEV)[None, :] < p["npl"].clamp(max=T)[:, None]
    few = ((tiles * listed).sum(1) * 2 * (16 // G) < k).sum().item()
    assert scan.last_redone(1300) <= few


def test_withheld_form_keeps_the_seeded_form():
    from torchpq_amd import kernels as K
    p = _big(32, 1024, 12, 2, ragged=False)
    assert _gate(p, 10)
    scan = K.IVFPQTopkHip(m=64)
    cs, sz = p["start"][p["cells"]].contiguous(), p["sizes"][p["cells"]].contiguous()
    pk = K.PackCodesHip()(p["storage"])
    args = (p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], 10)
    kw = dict(packed=pk, slots_hint=int(p["sizes"].float().mean().item() * 12), cells=p["cells"], n_cells=16)
    a = scan.topk_fused(*args, **kw)
    assert scan.last_cell_threshold() is True
    b = scan.topk_fused(*args, cell_threshold=False, **kw)
    assert scan.last_cell_major() is True and scan.last_cell_threshold() is False
    torch.cuda.synchronize()
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


def test_integer_data_mass_ties_at_the_kth_place():
    p = _big(33, 1100, 12, 2, integer=True)
    _check(p, 100)
    _check(p, 10, "inner")


def test_probe_repeated_across_the_first_pass_boundary():
    """probe T is probe T - 1 again for a third of the queries, probe T - 1 is probe T - 2 again for another third: the
    repeat is skipped by both passes as the scan skips it"""
    p = _big(34, 1100, 12, 2, ragged=False)
    q = torch.arange(1100, device=DEV)
    p["cells"][q % 3 == 0, T] = p["cells"][q % 3 == 0, T - 1]
    p["cells"][q % 3 == 1, T - 1] = p["cells"][q % 3 == 1, T - 2]
    scan = _check(p, 100)
    assert scan.last_redone(1100) == 0


def test_nan_inf_queries_and_a_cell_out_of_range():
    nq = 1100
    p = _big(35, nq, 12, 2, ragged=False)
    p["query"][3, 7] = float("nan")
    p["query"][:, 8] = float("inf")
    p["query"][5, 9] = 1e30       # beyond the fp16 scale's range: the exact kernel's
    p["query"][:, 10] = 0.0
    scan = _check(p, 50, nan_rows=[7, 8, 9])
    assert 4 <= scan.last_redone(nq) < 4 + nq // 10
    # a cell id out of range flags its query -- in the first pass's probes or behind them
    p["cells"][20, 1] = 16
    p["cells"][21, 11] = -1
    scan = _check(p, 50, nan_rows=[7, 8, 9])
    assert 6 <= scan.last_redone(nq) < 6 + nq // 10


def test_a_cell_whose_maxima_exceed_the_list():
    """one cell of 20 000 slots among the first probes of every query: 625 tiles x 2 half-lanes x 16 / G maxima, beyond the
    1 024 entries of the list -- the rest is dropped, a subset still bounds"""
    sizes = [20000] + SIZES[1:] + SIZES
    p = _big(36, 1024, 12, 2, sizes=sizes, ragged=False)
    p["cells"][:, 0] = 0
    for c in range(1, 12):     # (the other probes: eleven different cells of 1 ... 15)
        p["cells"][:, c] = 1 + (torch.arange(1024, device=DEV) + c) % 15
    assert 625 * 2 * (16 // G) > 1024
    scan = _check(p, 100)
    assert scan.last_redone(1024) == 0


def test_fewer_than_k_maxima_in_the_first_cells():
    """the first T cells hold a few slots each: the threshold is -inf, every live slot behind them is admitted, and fits
    (the slots hint is the caller's estimate: it is what takes the form here)"""
    sizes = [3, 5, 2, 7, 1, 4, 6, 2] + [200] * 8
    p = _big(37, 1024, 12, 2, sizes=sizes, ragged=False, holes=False)
    p["cells"] = torch.arange(12, device=DEV).repeat(1024, 1).contiguous()
    p["hint"] = 12 * 600
    scan = _check(p, 100)
    assert scan.last_redone(1024) == 0


def test_graphed_search_replays_the_form():
    from torchpq_amd.index import IVFPQIndex
    rng = np.random.default_rng(38)
    d, n, nq, k, n_cells = 64, 16000, 1024, 10, 16
    centers = rng.standard_normal((d, n_cells)) * 4
    base = (centers[:, rng.integers(0, n_cells, n)] + rng.standard_normal((d, n))).astype(np.float32)
    np.random.seed(38)
    idx = IVFPQIndex(d_vector=d, n_subvectors=64, n_cells=n_cells, initial_size=1024, device=DEV, verbose=0)
    x = torch.from_numpy(base).to(DEV)
    idx.train(x)
    idx.add(x)
    idx.n_probe = 12
    idx.use_smart_probing = False
    xq = x[:, :nq].contiguous() + 0.05
    scan = idx._ivfpq_topk._scan
    v, i = idx.search(xq, k=k)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_threshold() is True
    idx.use_cell_threshold = False
    v0, i0 = idx.search(xq, k=k)
    assert scan.last_cell_major() is True and scan.last_cell_threshold() is False
    assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(i, i0)
    idx.use_cell_threshold = True
    gs = idx.graphed_search(nq, k=k)
    v1, i1 = (t.clone() for t in gs(xq))
    v2, i2 = (t.clone() for t in gs(xq))
    torch.cuda.synchronize()
    assert scan.last_cell_threshold() is True
    assert torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(i1, i)
    assert torch.equal(v2.view(torch.int32), v1.view(torch.int32)) and torch.equal(i2, i1)


def test_form_under_guarded_prefilled_allocations(monkeypatch):
    """the form's whole call with every buffer the wrapper allocates -- the workspace above all -- between guard bands and
    pre-filled with 0x00 and with 0xFF: the same bits as the reference-layout kernel either way, no guard touched.  (thr
    is written for every query before pass B reads it, cell_kth_kernel reads only what pass A wrote, and the pads and
    counters are the seed kernel's: nothing of the form depends on what the workspace held)"""
    from guarded_alloc import run_guarded
    from torchpq_amd import kernels as K
    p = _big(40, 1100, 12, 2, ragged=True)
    assert _gate(p, 100)
    p["packed"] = K.PackCodesHip()(p["storage"])
    ref, _ = _search(p, 100, cells=False, packed=False)

    def go():
        got, scan = _search(p, 100)
        assert scan.last_cell_threshold() is True
        return got
    for fill, got in run_guarded(go, monkeypatch=monkeypatch).items():
        assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32)), fill
        assert torch.equal(got[1], ref[1]), fill


@pytest.mark.parametrize("ds,distance", [(2, "euclidean"), (1, "inner")])
def test_first_pass_against_float64(ds, distance):
    """Pass A read back from the kept workspace of a whole call (IVFPQTopkHip.last_cell_threshold_state): 1 024 queries
    -- the route's smallest batch -- over 8 cells of ~660 slots, ragged probe counts, k = 20.  Every maximum that
    survived the candidate pass is within delta_q of the exact (float64) value of a live row of the query's first T
    probes, and the best live row of those probes is among them when all survived; the counts are what the tiling says;
    M_k - delta_q <= the exact k-th best over all listed probes, M_k taken from the maxima where all survived and from the
    stored threshold (M_k - 2 delta_q, unfolded) for every query.  Tombstones and the slack rows behind every cell decode to
    the zero vector and the queries are short, so under the euclidean metric a dead row would be the best of its group
    by far: none shows."""
    from torchpq_amd._lib import load
    nq, n_cells, n_probe, k = 1024, 8, 8, 20
    p = _big(41 + ds, nq, n_probe, ds, ragged=True)
    assert 5000 <= p["n_slots"] <= 7000 and _gate(p, k)
    p["query"] = p["query"] * 0.03
    p["codebook"][:, :, 255] = 0.0
    st, size, emp = p["start"].cpu().numpy(), p["sizes"].cpu().numpy(), p["is_empty"].cpu().numpy()
    dead = emp != 0
    for c in range(n_cells):
        dead[st[c] + size[c]:st[c] + size[c] + 5] = True
    dead_t = torch.from_numpy(dead).to(DEV)
    p["storage"] = torch.where(dead_t[None, :, None], torch.full_like(p["storage"], 255),
                               torch.clamp(p["storage"], max=254)).contiguous()
    got, scan = _search(p, k, distance)
    assert scan.last_cell_threshold() is True
    state = {name: t.cpu().numpy() for name, t in scan.last_cell_threshold_state().items()}
    count, maxima, survived, thr, band, cand = (state[n] for n in ("count", "maxima", "survived", "threshold", "band",
                                                                   "candidates"))
    cb = p["codebook"].double().cpu().numpy()
    codes = p["storage"].permute(1, 0, 2).reshape(p["n_slots"], 64).cpu().numpy().astype(np.int64)
    xhat = cb[np.arange(64)[None, :], :, codes].reshape(p["n_slots"], 64 * ds)
    q = p["query"].double().cpu().numpy().T
    q2 = (q ** 2).sum(1)
    exact = (2 * q @ xhat.T - q2[:, None] - (xhat ** 2).sum(1)[None, :]) if distance == "euclidean" else q @ xhat.T
    cells, npl = p["cells"].cpu().numpy(), p["npl"].cpu().numpy()
    fold = load().tpq_ivfpq_cell_fold_threshold
    whole = 0
    for qi in range(nq):
        first = np.zeros(p["n_slots"], bool)
        listed = np.zeros(p["n_slots"], bool)
        tiles = 0
        for c in cells[qi, :npl[qi]]:
            listed[st[c]:st[c] + size[c]] = True
        for c in cells[qi, :min(npl[qi], T)]:
            first[st[c]:st[c] + size[c]] = True
            tiles += (size[c] + 31) // 32
        first &= ~dead
        listed &= ~dead
        assert count[qi] == tiles * 2 * (16 // G)
        assert band[qi] > 0, "a query redone exactly: the shape is meant to fit"
        delta = band[qi] / 2.0
        n = min(count[qi], maxima.shape[1])
        assert np.isinf(maxima[qi, n:]).all()
        kept = maxima[qi, :n][survived[qi, :n]]
        kept = kept[~np.isnan(kept)].astype(np.float64)
        ex = np.sort(exact[qi, first])
        if len(kept):
            pos = np.clip(np.searchsorted(ex, kept), 1, len(ex) - 1) if len(ex) > 1 else np.zeros(len(kept), int)
            near = np.minimum(np.abs(ex[pos] - kept), np.abs(ex[np.maximum(pos - 1, 0)] - kept))
            assert (near <= delta).all(), (qi, near.max(), delta)
        all_ex = np.sort(exact[qi, listed])
        kth = all_ex[-k] if len(all_ex) >= k else -np.inf
        if survived[qi, :n].all():
            whole += 1
            # a group without a live row stores nothing: at most one group per live row, at least one per G of them
            assert (first.sum() + G - 1) // G <= len(kept) <= first.sum()
            if len(kept):
                assert abs(kept.max() - ex[-1]) <= delta       # the best live row is the best of its group
            m_k = np.sort(kept)[-k] if len(kept) >= k else -np.inf
            assert m_k - delta <= kth
            want = np.float32(np.float32(m_k) - band[qi])
            if distance == "euclidean" and np.isfinite(want):
                q2f = np.float32(q2[qi])
                assert abs(float(thr[qi]) - float(fold(want, q2f))) <= 1e-5 * (abs(float(want)) + float(q2f))
            else:
                assert thr[qi] == want
        # every query, from the stored threshold: thr unfolded is M_k - 2 delta_q (to a rounding of |q|^2)
        t = float(thr[qi]) - (q2[qi] if distance == "euclidean" else 0.0)
        assert t + delta - 1e-5 * (abs(t) + q2[qi]) <= kth or np.isinf(t)
        assert cand[qi] >= min(k, listed.sum())
    assert whole >= nq // 2, "the shape is meant to keep most queries' maxima whole"
