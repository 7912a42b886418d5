"""GPU: the cell-major form of the m = 64 large-batch scan route (csrc/scan_cells.hip: threshold pass over the first P0
probes, seeds, inversion of the probe table, fp16 matrix-core candidates per cell, the route's own finish kernel and
exact redo) against the reference-layout kernel (`packed=None`), values bit for bit and addresses entry for entry; and
the candidate pass on its own against float64 numpy."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
P0 = 4
SIZES = [0, 1, 63, 64, 65, 255, 257, 300]


def _problem(seed, nq, n_cells, n_probe, ds, sizes=None, integer=False, holes=True, ragged=True):
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    m = 64
    sizes = torch.tensor((sizes or SIZES * (n_cells // 8))[:n_cells], device=DEV, dtype=torch.long)
    cap = sizes + 5
    start = torch.cumsum(cap, 0) - cap
    n_slots = int(cap.sum().item())
    storage = torch.randint(0, 256, (m // 4, n_slots, 4), generator=g, device=DEV, dtype=torch.uint8)
    if integer:   # small integers: every value is exact in any order, mass ties at the k-th place
        codebook = torch.randint(-2, 3, (m, ds, 256), generator=g, device=DEV).float()
        query = torch.randint(-2, 3, (m * ds, nq), generator=g, device=DEV).float()
    else:
        codebook = torch.randn(m, ds, 256, generator=g, device=DEV) * 3
        query = torch.randn(m * ds, nq, generator=g, device=DEV) * 3
    is_empty = (torch.rand(n_slots, generator=g, device=DEV) < 0.05).to(torch.uint8) if holes else None
    cells = torch.rand(nq, n_cells, generator=g, device=DEV).argsort(1)[:, :n_probe].contiguous()
    npl = torch.full((nq,), n_probe, device=DEV, dtype=torch.long)
    if ragged:
        npl = torch.randint(0, n_probe + 1, (nq,), generator=g, device=DEV)
        npl[:8] = torch.tensor([0, 1, P0 - 1, P0, P0 + 1, n_probe, n_probe, n_probe], device=DEV)
    return dict(storage=storage, codebook=codebook, query=query, is_empty=is_empty, cells=cells, npl=npl,
                start=start, sizes=sizes, n_cells=n_cells, n_slots=n_slots)


def _search(p, k, distance="euclidean", cells=True, packed=True, scan=None):
    from torchpq_amd import kernels as K
    scan = scan or K.IVFPQTopkHip(m=64)
    scan.keep_workspace = True
    cs, sz = p["start"][p["cells"].clamp(0, p["n_cells"] - 1)].contiguous(), p["sizes"][
        p["cells"].clamp(0, p["n_cells"] - 1)].contiguous()
    if "sz" in p:   # (a problem that hands its probes' sizes over itself: void probes, test_gpu_scan_cells_edges.py)
        sz = p["sz"]
    hint = p.get("hint") or int(p["sizes"].float().mean().item() * p["cells"].shape[1])
    pk = p.setdefault("packed", K.PackCodesHip()(p["storage"])) if packed else None
    out = scan.topk_fused(p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], k,
                          distance=distance, packed=pk, slots_hint=hint,
                          cells=p["cells"] if cells else None, n_cells=p["n_cells"])
    torch.cuda.synchronize()
    return out, scan


def _check(p, k, distance="euclidean", expect_form=True, nan_rows=None):
    got, scan = _search(p, k, distance)
    assert scan.last_route() == "dump_sel16"
    assert scan.last_cell_major() is expect_form
    ref, _ = _search(p, k, distance, cells=False, packed=False)
    ok = torch.ones(got[0].shape[0], dtype=torch.bool, device=DEV)
    if nan_rows is not None:   # (NaN values compare unequal to themselves: those rows are checked through the addresses)
        ok[nan_rows] = False
    assert torch.equal(got[0][ok].view(torch.int32), ref[0][ok].view(torch.int32))
    assert torch.equal(got[1], ref[1])
    return scan


CASES = [  # nq, n_cells, n_probe, ds, distance, k
    (1024, 8, P0 + 1, 2, "euclidean", 100), (1024, 8, 8, 1, "inner", 10), (1024, 16, P0 + 1, 1, "euclidean", 1),
    (1024, 16, 8, 2, "inner", 128), (1025, 8, P0 + 1, 1, "inner", 128), (1025, 8, 8, 2, "euclidean", 10),
    (1025, 16, P0 + 1, 2, "inner", 100), (1025, 16, 8, 1, "euclidean", 100), (1300, 8, P0 + 1, 2, "euclidean", 1),
    (1300, 8, 8, 1, "euclidean", 128), (1300, 16, P0 + 1, 1, "inner", 10), (1300, 16, 8, 2, "euclidean", 100),
]


@pytest.mark.parametrize("nq,n_cells,n_probe,ds,distance,k", CASES)
def test_equals_the_reference_layout_kernel(nq, n_cells, n_probe, ds, distance, k):
    """cell sizes 0, 1, 63, 64, 65, 255, 257, 300; ragged probe lists with values <= P0; tombstones"""
    p = _problem(nq + n_cells + n_probe + k, nq, n_cells, n_probe, ds)
    scan = _check(p, k, distance)
    # (a query whose first cells hold fewer than k entries admits everything else: the few whose lists overflow are redone)
    assert scan.last_redone(nq) < nq // 10


def test_cells_probed_by_1_127_128_and_129_queries():
    """cells listed by 1, 127, 128 and 129 queries: a candidate block takes a group of 32 (kCellGroup), so these are one
    short group, three full groups and a group of 31, four full groups, four and a group of one (the edges of a single
    group -- 31, 32, 33 -- are test_gpu_scan_cells_edges.py's)"""
    nq, n_cells, n_probe = 1300, 16, 8
    p = _problem(5, nq, n_cells, n_probe, 2, ragged=False)
    g = torch.Generator(device=DEV)
    g.manual_seed(6)
    p["cells"] = torch.rand(nq, 12, generator=g, device=DEV).argsort(1)[:, :n_probe].contiguous()   # cells 0..11
    first = 0
    for cell, count in ((12, 1), (13, 127), (14, 128), (15, 129)):
        p["cells"][first:first + count, n_probe - 1] = cell
        first += count
    listed = torch.bincount(p["cells"][:, P0:].reshape(-1), minlength=n_cells)
    assert listed[12:].tolist() == [1, 127, 128, 129]
    _check(p, 100)


def test_integer_data_mass_ties_at_the_kth_place():
    p = _problem(11, 1100, 8, 8, 2, integer=True)
    _check(p, 100)
    _check(p, 10, "inner")


def test_fewer_than_k_entries_in_the_first_cells():
    """the threshold is -inf: everything of the other cells is admitted, and fits"""
    p = _problem(12, 1024, 8, 8, 2, sizes=[3, 5, 2, 7, 1, 120, 130, 140], ragged=False, holes=False)
    p["cells"] = torch.arange(8, device=DEV).repeat(1024, 1).contiguous()
    scan = _check(p, 100)
    assert scan.last_redone(1024) == 0


def test_candidate_overflow_is_flagged_and_redone():
    """all queries identical, the first cells hold fewer than k entries, one cell of 3 000 slots: more candidates than
    the lists hold -- every query is flagged and redone by the exact kernel, to the same bits"""
    p = _problem(13, 1024, 8, 8, 2, sizes=[3, 5, 2, 7, 3000, 10, 10, 10], ragged=False)
    p["cells"] = torch.arange(8, device=DEV).repeat(1024, 1).contiguous()
    p["query"] = p["query"][:, :1].repeat(1, 1024).contiguous()
    scan = _check(p, 100)
    assert scan.last_redone(1024) == 1024


def test_nan_inf_queries_and_a_cell_out_of_range():
    nq = 1100
    p = _problem(14, nq, 16, 8, 2, ragged=False)
    p["query"][3, 7] = float("nan")
    p["query"][:, 8] = float("inf")
    p["query"][5, 9] = 1e30       # beyond the fp16 scale's range: the exact kernel's
    p["query"][:, 10] = 0.0
    scan = _check(p, 50, nan_rows=[7, 8, 9])
    assert scan.last_redone(nq) >= 4
    # a cell id out of range flags its query; the extents it came with are still those of a real cell
    p["cells"][20, 6] = 16
    p["cells"][21, 7] = -1
    scan = _check(p, 50, nan_rows=[7, 8, 9])
    assert scan.last_redone(nq) >= 6


def test_withheld_cells_keep_the_query_major_path():
    p = _problem(15, 1024, 8, 8, 2)
    got, scan = _search(p, 100, cells=False)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is False
    ref, _ = _search(p, 100, cells=False, packed=False)
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])


def test_graphed_search_replays_the_form():
    from torchpq_amd.index import IVFPQIndex
    rng = np.random.default_rng(16)
    d, n, nq, k = 64, 6000, 1024, 10
    centers = rng.standard_normal((d, 8)) * 4
    base = (centers[:, rng.integers(0, 8, n)] + rng.standard_normal((d, n))).astype(np.float32)
    np.random.seed(16)
    idx = IVFPQIndex(d_vector=d, n_subvectors=64, n_cells=8, initial_size=1024, device=DEV, verbose=0)
    x = torch.from_numpy(base).to(DEV)
    idx.train(x)
    idx.add(x)
    idx.n_probe = 8
    idx.use_smart_probing = False
    xq = x[:, :nq].contiguous() + 0.05
    scan = idx._ivfpq_topk._scan
    v, i = idx.search(xq, k=k)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is True
    idx.use_cell_major = False
    v0, i0 = idx.search(xq, k=k)
    assert scan.last_cell_major() is False
    assert torch.equal(v.view(torch.int32), v0.view(torch.int32)) and torch.equal(i, i0)
    idx.use_cell_major = True
    gs = idx.graphed_search(nq, k=k)
    v1, i1 = (t.clone() for t in gs(xq))
    v2, i2 = (t.clone() for t in gs(xq))
    torch.cuda.synchronize()
    assert torch.equal(v1.view(torch.int32), v.view(torch.int32)) and torch.equal(i1, i)
    assert torch.equal(v2.view(torch.int32), v1.view(torch.int32)) and torch.equal(i2, i1)


@pytest.mark.parametrize("ds,distance", [(2, "euclidean"), (1, "inner")])
def test_candidate_kernel_against_float64(ds, distance):
    """returned set contains every slot whose exact value is >= tau, every returned slot has exact >= tau - 2 delta and
    a value within delta of the exact one, no duplicates, counts match; exact = the sum in float64"""
    from torchpq_amd import kernels as K
    nq, n_cells, n_probe = 300, 8, 6
    p = _problem(17 + ds, nq, n_cells, n_probe, ds, ragged=True)     # 1 045 slots
    assert p["n_slots"] <= 2000
    cs = p["start"][p["cells"]].contiguous()
    sz = p["sizes"][p["cells"]].contiguous()
    cb = p["codebook"].double().cpu().numpy()                        # [m, ds, 256]
    codes = p["storage"].permute(1, 0, 2).reshape(p["n_slots"], 64).cpu().numpy().astype(np.int64)
    xhat = cb[np.arange(64)[None, :], :, codes].reshape(p["n_slots"], 64 * ds)   # [slot, m * ds]
    q = p["query"].double().cpu().numpy().T                                         # [nq, m * ds]
    if distance == "euclidean":
        exact = -((q[:, None, :] - xhat[None, :, :]) ** 2).sum(-1)
    else:
        exact = q @ xhat.T
    live = np.zeros((nq, p["n_slots"]), bool)
    cells, npl = p["cells"].cpu().numpy(), p["npl"].cpu().numpy()
    st, size, emp = p["start"].cpu().numpy(), p["sizes"].cpu().numpy(), p["is_empty"].cpu().numpy()
    first = 1
    for qi in range(nq):
        for c in cells[qi, first:npl[qi]]:
            live[qi, st[c]:st[c] + size[c]] = True
    live &= emp[None, :] == 0
    # thresholds: the 20th best exact value of the listed slots (fewer: -inf)
    masked = np.where(live, exact, -np.inf)
    tau = np.sort(masked, 1)[:, -20].astype(np.float32)
    count, values, address, band, flags = K.CellCandidatesHip()(
        p["storage"], p["query"], p["codebook"], p["cells"], n_cells, cs, sz, p["npl"],
        torch.from_numpy(tau).to(DEV), first_probe=first, capacity=2048, is_empty=p["is_empty"], distance=distance)
    torch.cuda.synchronize()
    count, values, address, band, flags = (t.cpu().numpy() for t in (count, values, address, band, flags))
    assert not flags.any()
    for qi in range(nq):
        got = address[qi, :count[qi]]
        # the returned value is the selection key: within delta_q = band / 2 of the exact one
        assert (np.abs(values[qi, :count[qi]].astype(np.float64) - exact[qi, got]) <= band[qi] / 2.0).all()
        assert (address[qi, count[qi]:] == -1).all()
        assert len(set(got.tolist())) == len(got), "duplicates"
        assert live[qi, got].all()
        must = set(np.nonzero(live[qi] & (exact[qi] >= tau[qi]))[0].tolist())
        assert must <= set(got.tolist())
        assert (exact[qi, got] >= np.float64(tau[qi]) - np.float64(band[qi])).all()
        assert band[qi] > 0
