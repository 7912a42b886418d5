"""GPU: the cell-major IVFFlat scan (tpq_ivf_flat_cells_topk, csrc/scan_flat_cells.hip) against tests/ivfflat_oracle.py
-- values bit-equal, addresses equal, no query redone unless the case asks for it -- and IVFFlatIndex with the switch on
against the same index with the switch off."""
import numpy as np
import pytest
import torch

import guarded_alloc
import ivfflat_cells_guarded
import ivfflat_oracle as forc
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu

# the edges of the candidate kernel's 256-row chunk and of its 64-row waves; 1 261 slots in all
CELL_SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 300)
CAND_CAP = 2048   # above every slot of a case: no query can overflow


def _case(seed, d, nq, n_probe, tomb=25, dup=True, scale=1.0, base=0.0, same=False, full=False):
    """cells 0 ... 6 are dealt at random; cell 8 (300 slots) is listed last by exactly min(129, nq - 1) queries -- one
    more than a block of 128 -- and cell 7 (257 slots) by exactly one; query 1 lists a cell twice in a row, query 0 one
    twice with another between"""
    rng = np.random.default_rng(seed)
    sizes = np.array(CELL_SIZES, np.int64)
    caps = sizes + rng.integers(1, 9, len(sizes))
    start = (np.cumsum(caps) - caps).astype(np.int64)
    cap = int(caps.sum())
    vectors = (base + scale * rng.standard_normal((d, cap))).astype(np.float32)   # free slots hold finite junk
    query = (base + scale * rng.standard_normal((d, nq))).astype(np.float32)
    is_empty = np.ones(cap, np.uint8)
    for c in range(len(sizes)):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    live = np.flatnonzero(is_empty == 0)
    if dup:   # a third of the slots hold one of five vectors: ties everywhere, the k-th place included
        src = rng.choice(live, 5, replace=False)
        dst = rng.choice(live, len(live) // 3, replace=False)
        vectors[:, dst] = vectors[:, src[rng.integers(0, 5, len(dst))]]
        query[:, 0] = vectors[:, src[0]]
    if same:
        vectors[:] = vectors[:, :1]
    if tomb:
        is_empty[rng.choice(live, tomb, replace=False)] = 1
    cells = np.stack([rng.permutation(7)[:n_probe] for _ in range(nq)])
    n_a = min(129, nq - 1)
    cells[:n_a, -1] = 8
    cells[nq - 1, -1] = 7
    if n_probe >= 4:
        cells[1, 1] = cells[1, 0]
        cells[0, 2] = cells[0, 0]
    npl = rng.integers(0, n_probe + 3, nq).astype(np.int64)   # 0, below, at and beyond max_nprobe
    npl[:max(n_a, nq // 2)] = n_probe
    npl[nq - 1] = n_probe + 2
    if full:
        npl[:] = n_probe
    return dict(vectors=vectors, query=query, is_empty=is_empty, cells=cells, cs=start[cells], sz=sizes[cells], npl=npl)


def _run(case, k, distance, first_probe, cand_cap=CAND_CAP, fill=None):
    from torchpq_amd.kernels import IVFFlatCellTopkHip
    op = IVFFlatCellTopkHip(first_probe=first_probe, cand_cap=cand_cap)
    op.fill_workspace = fill
    v, a = op(T(case["vectors"]), T(case["query"]), T(case["cs"]), T(case["sz"]), T(case["npl"]), k,
              is_empty=T(case["is_empty"]), distance=distance, cells=T(case["cells"]), n_cells=len(CELL_SIZES))
    assert op.last_route == "cell_major"
    return N(v), N(a), op


def _check(case, k, distance, first_probe, redone=0, rows=None, **kw):
    v, a, op = _run(case, k, distance, first_probe, **kw)
    ev, ea = forc.scan_topk(case["vectors"], case["query"], case["is_empty"], case["cs"], case["sz"], case["npl"], k,
                            "euclidean" if distance == "euclidean" else "inner")
    rows = slice(None) if rows is None else rows
    assert v.shape == ev.shape and v.dtype == np.float32 and a.dtype == np.int64
    assert np.array_equal(a[rows], ea[rows])
    assert np.array_equal(v[rows].view(np.uint32), ev[rows].view(np.uint32))
    assert op.last_redone == redone, op.last_redone      # (the fallback would hide a broken candidate kernel)
    return v, a


# (d, nq, n_probe, first_probe, k, distance): n_probe below, at and above first_probe; k = 256 is above the live
# candidates of some rows
OP_CASES = [
    (1, 3, 4, 1, 1, "euclidean"),
    (1, 1000, 6, 2, 100, "inner"),
    (24, 130, 6, 2, 100, "euclidean"),
    (24, 1000, 4, 1, 256, "inner"),
    (24, 3, 2, 2, 100, "euclidean"),
    (24, 130, 1, 2, 1, "inner"),
    (128, 130, 6, 4, 256, "euclidean"),
    (128, 1000, 6, 2, 100, "euclidean"),
    (128, 3, 4, 1, 100, "inner"),
    (960, 3, 4, 2, 100, "euclidean"),
    (960, 130, 4, 1, 1, "inner"),
]


@pytest.mark.parametrize("d,nq,n_probe,first_probe,k,distance", OP_CASES)
def test_op_against_the_oracle(d, nq, n_probe, first_probe, k, distance):
    case = _case(1000 * d + nq + n_probe, d, nq, n_probe, scale=0.25 if d >= 960 else 1.0)
    listed = case["cells"][np.arange(n_probe)[None, :] < case["npl"][:, None]]
    assert (listed == 8).sum() == min(129, nq - 1) and (listed == 7).sum() == 1
    v, a = _check(case, k, distance, first_probe)
    assert np.all(v[a < 0] == -np.inf) and np.all(v[:, 1:] <= v[:, :-1])
    if k == 256 and nq > 130:     # (with 130 queries every row lists all its probes)
        assert (a >= 0).sum(1).min() < k


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
@pytest.mark.parametrize("k", [10, 100])
def test_the_band_holds_under_cancellation(k, distance):
    """components 1000 + 0.01 N(0, 1), d = 128.  Modelled on the CPU in float64 (1 200 slots, 40 queries): the fast value
    2 dot - |x|^2 - |q|^2 is up to 216 away from the chain's value where all values lie within 0.025 of each other
    (euclidean; inner product: up to 32, four ulps of the k-th value), and the band, 1.2e4, holds EVERY slot of the case
    around the k-th value for k = 10 and k = 100 alike: the candidate kernel admits all of them and the order is the
    finish kernel's alone."""
    _check(_case(7 + k, 128, 40, 6, scale=0.01, base=1000.0), k, distance, 2)


def test_overflow_redoes_every_query():
    """every slot holds the same vector: all values tie with the threshold, every list overflows 64 entries"""
    case = _case(3, 24, 20, 6, dup=False, same=True, full=True)
    _check(case, 10, "euclidean", 1, redone=20, cand_cap=64)


def test_nan_and_inf_queries_are_redone_and_a_dirty_workspace_changes_nothing():
    from torchpq_amd.kernels import IVFFlatTopkHip
    case = _case(11, 24, 130, 6)
    clean = _check(case, 100, "euclidean", 2, fill=0xFF)
    case["query"][5, 3] = np.nan
    case["query"][7, 100] = np.inf
    keep = np.setdiff1d(np.arange(130), [3, 100])
    v, a = _check(case, 100, "euclidean", 2, redone=2, rows=keep, fill=0xFF)
    assert np.array_equal(a[keep], clean[1][keep])
    ev, ea = IVFFlatTopkHip()(T(case["vectors"]), T(case["query"]), T(case["cs"]), T(case["sz"]), T(case["npl"]), 100,
                              is_empty=T(case["is_empty"]), distance="euclidean")
    for q in (3, 100):
        assert np.array_equal(a[q], N(ea)[q]) and np.array_equal(v[q].view(np.uint32), N(ev)[q].view(np.uint32))


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_index_with_the_switch_on_equals_the_switch_off(distance):
    from torchpq_amd.index import IVFFlatIndex
    base, queries = _clustered(4, 24, 3000, 300)
    torch.manual_seed(0)
    np.random.seed(0)
    idx = IVFFlatIndex(24, n_cells=16, initial_size=64, distance=distance, device=DEV)
    idx.train(T(base))
    ids = idx.add(T(base))
    idx.remove(ids=ids[::20])
    idx.n_probe = 6
    idx.cell_major_min_batch = 1
    for k, route in ((1, "cell_major"), (100, "cell_major"), (300, "query_major")):
        idx.use_cell_major = False
        want = idx.search(T(queries), k=k, return_address=True)
        assert idx.last_route == "query_major"
        idx.use_cell_major = True
        got = idx.search(T(queries), k=k, return_address=True)
        assert idx.last_route == route
        assert torch.equal(got[0].view(torch.int32), want[0].view(torch.int32))
        assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


def test_cell_major_inside_guarded_buffers(monkeypatch):
    """the case of tests/ivfflat_cells_guarded.py with the outputs and the workspace between canaries: the guards stay
    intact, and the results are the same bits from 0x00- and 0xFF-filled buffers"""
    out = guarded_alloc.run_guarded(ivfflat_cells_guarded.build(), monkeypatch=monkeypatch)
    for s, t in zip(out[0x00], out[0xFF]):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.view(torch.uint8), t.view(torch.uint8))
