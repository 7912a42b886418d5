"""GPU: the kept state of the cell-major scan (csrc/scan_cells.hip, `The kept state`; tpq_ivfpq_search_fused_cells_kept;
IVFPQIndex.use_cell_kept): what the form derives from codes, codebook and tombstones alone -- scale and bound, the split
codebook as the candidate kernels stage it, a norm per slot address -- built by the first search and read by the others.
Results against the reference-layout kernel (`packed=None`) and against the per-call path, bit for bit; the state itself
against what a per-call search leaves in its workspace and against the numpy restatement of the split; staleness on
IVFPQIndex; GraphedSearch; the new entry point under guarded, pre-filled allocations.
Shapes: the grid of tests/test_gpu_scan_cell_threshold.py -- the smallest the form is taken at."""
import numpy as np
import pytest
import torch

import cell_kept_cases as ck
import guarded_alloc as ga
from test_gpu_guarded_buffers import BUILDERS, _nothing_after_a_gpu_fault, same_bits
from test_gpu_scan_cell_threshold import _big, _gate
from test_gpu_scan_cells import DEV, _search
from test_scan_cell_maxima_cpu import T

pytestmark = pytest.mark.gpu

CASES = [  # nq, n_probe, ds, distance, k, threshold form
    (1024, T + 1, 2, "euclidean", 100, True), (1024, 12, 1, "inner", 10, True), (1025, T + 1, 1, "euclidean", 1, True),
    (1300, 12, 2, "inner", 128, True), (1025, 12, 2, "euclidean", 10, False), (1300, T + 1, 1, "inner", 100, False),
    (1024, 12, 1, "euclidean", 128, False), (1300, T + 1, 2, "inner", 1, False),
]


def _equal(a, b):
    return torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("nq,n_probe,ds,distance,k,thr", CASES)
def test_kept_equals_per_call_and_the_reference_layout_kernel(nq, n_probe, ds, distance, k, thr):
    """the call that builds, a call that reuses and a third on another stream, threshold form and seeded form: values bit
    for bit and addresses entry for entry against the reference-layout kernel and against the call without a state; one
    build.  Every call here is followed by a device-wide synchronize (ck.run), so the third call shows that the path
    runs from another stream and waits on the build's event without error; it does NOT show that the event is what
    orders it -- the build had completed before it was issued"""
    p = _big(nq + n_probe + k, nq, n_probe, ds, k=k, ragged=False)
    assert _gate(p, k)
    ref, _ = _search(p, k, distance, cells=False, packed=False)
    plain, scan = ck.run(p, k, distance, cell_threshold=thr)
    assert scan.last_cell_major() is True and scan.last_cell_threshold() is thr and scan.last_cell_kept is None
    assert _equal(plain, ref)
    kept = ck.Provider()
    for want in ("built", "reused"):
        got, scan = ck.run(p, k, distance, kept=kept, cell_threshold=thr)
        assert scan.last_cell_major() is True and scan.last_cell_threshold() is thr and scan.last_cell_kept == want
        assert _equal(got, ref) and _equal(got, plain)
        assert scan.last_redone(nq) == 0
    side = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(side):
        got, scan = ck.run(p, k, distance, kept=kept, cell_threshold=thr)
    assert scan.last_cell_kept == "reused" and _equal(got, ref)
    assert kept.state.builds == 1 and kept.asked == 3


def test_a_call_outside_the_form_asks_for_no_state():
    """fewer queries than the large-batch route takes: the library's rule (tpq_ivfpq_scan_cell_norms) says no, and no
    state is asked for, let alone allocated"""
    p = _big(5, 600, 12, 2, ragged=False)
    kept = ck.Provider()
    got, scan = ck.run(p, 10, kept=kept)
    assert scan.last_cell_major() is False and scan.last_cell_kept is None and kept.asked == 0 and kept.state is None
    assert _equal(got, _search(p, 10, cells=False, packed=False)[0])


def _workspace_views(scan, p, k):
    """(parameters f32 [4], norms f32 [n_slots]) a per-call search left in its kept workspace (csrc/scan_cells.h:
    cell_fill_extras behind the lists in use, the layout of the seeded form's first probe)"""
    from torchpq_amd import _lib
    ws, nq, n_probe = scan.last_workspace, p["query"].shape[1], p["cells"].shape[1]
    lists = lambda ch: 2 * ck.align(nq * 4) + nq * ch * 512 + ck.align(nq * ch * 4)  # noqa: E731
    extras = _lib.load().tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, p["n_cells"], 4)
    chunks = next(ch for ch in (16, 8) if (k + 63) // 64 < ch and scan.last_workspace_bytes >= lists(ch) + extras)
    at = lists(chunks)
    return (ws[at:at + 16].view(torch.float32).cpu().numpy(),
            ws[at + extras:at + extras + 4 * p["n_slots"]].view(torch.float32).cpu().numpy())


@pytest.mark.parametrize("ds,thr", [(1, True), (2, True), (2, False)])
def test_the_state_is_what_a_per_call_search_derives(ds, thr):
    """parameters and the norms of every slot of a listed cell, NaN for a tombstone, against the workspace of a search
    without a state; the codebook image against the numpy restatement of the split"""
    nq, n_probe, k = 1024, 12, 10
    p = _big(40 + ds, nq, n_probe, ds, ragged=False)
    _, scan = ck.run(p, k, cell_threshold=thr)
    assert scan.last_cell_norms() is True and scan.last_cell_threshold() is thr
    params, norms = _workspace_views(scan, p, k)
    kept = ck.Provider()
    ck.run(p, k, kept=kept, cell_threshold=thr)
    buf = kept.state.buf.cpu().numpy()
    assert buf.size == ck.kept_bytes(p["n_slots"], ds)
    kparams, image, knorms = ck.views(buf, p["n_slots"], ds)
    assert kparams.tobytes() == params.tobytes()
    assert kparams[3] == ck.scale(p["codebook"].cpu().numpy()) and kparams[2] == 1.0
    assert image.tobytes() == ck.split_image(p["codebook"].cpu().numpy()).tobytes()
    first = 0 if thr else 4                                    # (the seeded form lists the probes behind the first four)
    listed = torch.unique(p["cells"][:, first:]).cpu().numpy()
    start, sizes = p["start"].cpu().numpy(), p["sizes"].cpu().numpy()
    slots = np.concatenate([np.arange(start[c], start[c] + sizes[c]) for c in listed])
    assert len(listed) == p["n_cells"] and slots.size == sizes.sum()
    assert knorms[slots].tobytes() == norms[slots].tobytes()
    empty = p["is_empty"].cpu().numpy().astype(bool)
    assert np.array_equal(np.isnan(knorms), empty) and empty[slots].any()


def _index(seed, n, d=128, n_cells=16):
    from torchpq_amd.index import IVFPQIndex
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    x = torch.randn(d, n, generator=g, device=DEV)
    np.random.seed(seed)
    torch.manual_seed(seed)
    index = IVFPQIndex(d_vector=d, n_subvectors=64, n_cells=n_cells, initial_size=1024, device=DEV)
    index.vq_codec_max_iter = index.pq_codec_max_iter = 4
    index.train(x)
    index.add(x)
    index.n_probe = 12
    return index, x, g


def _fresh_like(index):
    """a freshly constructed index with the same content and no kept state"""
    from torchpq_amd.index import IVFPQIndex
    other = IVFPQIndex(d_vector=index.d_vector, n_subvectors=64, n_cells=index.n_cells, initial_size=1024, device=DEV)
    other.load_state_dict(index.state_dict())
    other.n_probe = index.n_probe
    other.use_cell_kept = False
    return other


def test_staleness_on_the_index():
    """add into existing cells, remove (tombstones), growth, load_state_dict of another index, a write to the codebook:
    after each, results equal those of a fresh index with the same content and use_cell_kept = False, and the build
    counter moved once per change, not per search"""
    index, x, g = _index(3, 12000)
    q = torch.randn(128, 1024, generator=g, device=DEV)
    scan = index._ivfpq_topk._scan

    def searched_twice(builds):
        for want in ("built", "reused"):
            got = index.search(q, k=10)
            assert scan.last_cell_major() is True and scan.last_cell_kept == want, (builds, want)
        assert index.cell_kept_builds == builds
        fresh = _fresh_like(index)
        ref = fresh.search(q, k=10)
        assert fresh._ivfpq_topk._scan.last_cell_kept is None and fresh.cell_kept_builds == 0
        torch.cuda.synchronize()
        assert _equal(got, ref), builds

    searched_twice(1)
    capacity = index._storage.shape[1]
    index.add(torch.randn(128, 200, generator=g, device=DEV))
    assert index._storage.shape[1] == capacity, "the first add fits the cells' spare room"
    searched_twice(2)
    index.remove(torch.arange(0, 3000, 7, device=DEV))
    searched_twice(3)
    index.add(torch.randn(128, 9000, generator=g, device=DEV))
    assert index._storage.shape[1] > capacity, "the container grew"
    searched_twice(4)
    other, _, _ = _index(4, 12500)
    index.load_state_dict(other.state_dict())
    searched_twice(5)
    index.pq_codec.codebook[3, 1, 17] += 0.25                  # in place: the tensor's version counter moves
    searched_twice(6)
    index.use_cell_kept = False
    index.search(q, k=10)
    assert scan.last_cell_kept is None and index.cell_kept_builds == 6


def test_graphed_search():
    """two replays equal the eager call; the warm-up searches built the state, the capture did not; a graph captured
    before an add refuses to replay"""
    index, x, g = _index(5, 12000)
    q = torch.randn(128, 1024, generator=g, device=DEV)
    eager = tuple(t.clone() for t in index.search(q, k=10))
    assert index.cell_kept_builds == 1
    index._drop_cell_kept()
    graphed = index.graphed_search(1024, k=10)
    scan = index._ivfpq_topk._scan
    assert index.cell_kept_builds == 2 and scan.last_cell_kept == "reused", "built by the warm-up, read by the capture"
    assert dict((n, i) for n, i in graphed._ident)["cell_kept"] is not None
    for _ in range(2):
        got = graphed(q)
        torch.cuda.synchronize()
        assert _equal(got, eager)
    assert index.cell_kept_builds == 2
    index.add(torch.randn(128, 50, generator=g, device=DEV))
    with pytest.raises(RuntimeError, match="changed since the graph was captured"):
        graphed(q)


@pytest.mark.parametrize("cid", sorted(ck.CASE_SYMBOLS))
def test_guards_hold_and_results_do_not_depend_on_the_fill(cid, monkeypatch):
    """a building call and a reusing call of tpq_ivfpq_search_fused_cells_kept: guards around the kept state and both
    workspaces hold, and the results do not depend on what the buffers held"""
    with _nothing_after_a_gpu_fault(cid):
        fn = BUILDERS[cid]()
        want = fn()
        torch.cuda.synchronize()
        got = ga.run_guarded(fn, monkeypatch=monkeypatch)
        for fill, out in got.items():
            same_bits(want, out, f"{cid}, fill {fill:#04x} against the plain call")
        same_bits(got[0x00], got[0xFF], f"{cid}, fill 0x00 against fill 0xff")
        n_slots = _big(71, 1025, 12, 2, ragged=True)["n_slots"]     # (the case's problem)
        sizes = [a.nbytes for a in ga.run_guarded.arenas[0xFF].allocations]
        assert sizes.count(ck.kept_bytes(n_slots, 2)) == 1, "one state for the two calls, allocated between guards"
