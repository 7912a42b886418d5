"""GPU: what the Python host layer promises around the library calls -- the diagnostics of the three packed scan entry
points (event pair, zero-query call, last_n_split / last_call / last_workspace) and the max_query_batch split of the
three IVF indexes."""
import math

import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import ivfpq_oracle as orc
from tests_support import N, T, _clustered

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

M, DS, K_TOP, N_PROBE, NQ = 8, 2, 10, 2, 3


@pytest.fixture(scope="module")
def scan_case():
    """4 cells of at most 100 slots (one empty), 3 queries probing 2 cells each; the oracle's answers, computed once"""
    import torchpq_amd.kernels as K
    from test_gpu_kernels import _random_index
    rng = np.random.default_rng(2024)
    sizes = np.array([100, 37, 0, 64], np.int64)
    storage, is_empty, start, _, a2i = _random_index(rng, M, 4, 0, sizes=sizes)
    cb = rng.standard_normal((M, DS, 256)).astype(np.float32)
    query = rng.standard_normal((M * DS, NQ)).astype(np.float32)
    cells = np.array([[0, 1], [3, 2], [1, 3]], np.int64)
    npl = np.full(NQ, N_PROBE, np.int64)
    lut = c_oracle.adc_lut(query, cb, "euclidean")
    part1 = orc.residual_part1(query, cb)
    part2 = (rng.standard_normal((4, M, 256)) * 5).astype(np.float32)
    base = rng.standard_normal((NQ, N_PROBE)).astype(np.float32)
    cs, sz = start[cells], sizes[cells]
    plain = c_oracle.scan_topk(storage, lut, is_empty, cs, sz, npl, K_TOP)
    resid = c_oracle.scan_topk_residual(storage, part1, part2, cells, base, is_empty, cs, sz, npl, K_TOP)
    st, p2 = T(storage), T(part2)
    slot_term, cell_bound = K.ResidualSlotTermsHip()(st, p2, T(start), T(sizes))
    g = dict(st=st, packed=K.PackCodesHip()(st), lut=T(lut), query=T(query), cb=T(cb), is_empty=T(is_empty),
             cs=T(cs), sz=T(sz), npl=T(npl), a2i=T(a2i), part1=T(part1), p2=p2, slot_term=slot_term,
             cell_bound=cell_bound, cells=T(cells), base=T(base))
    return dict(g=g, a2i=a2i, expect={"topk": plain, "topk_fused": plain, "topk_residual_packed": resid})


def _call(scan, entry, g, with_ids, nq=NQ):
    """the entry point on the first `nq` queries of the case"""
    a2i = g["a2i"] if with_ids else None
    cs, sz, npl = g["cs"][:nq], g["sz"][:nq], g["npl"][:nq]
    if entry == "topk":
        return scan.topk(g["st"], g["lut"][:, :nq].contiguous(), g["is_empty"], cs, sz, npl, n_candidates=K_TOP,
                         packed=g["packed"], address2id=a2i)
    if entry == "topk_fused":
        return scan.topk_fused(g["st"], g["query"][:, :nq].contiguous(), g["cb"], g["is_empty"], cs, sz, npl,
                               n_candidates=K_TOP, packed=g["packed"], address2id=a2i)
    return scan.topk_residual_packed(g["st"], g["packed"], g["p2"], g["slot_term"], g["cell_bound"],
                                     g["cells"][:nq], g["base"][:nq], g["is_empty"], cs, sz, npl,
                                     n_candidates=K_TOP, part1=g["part1"][:nq], address2id=a2i)


@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("entry", ["topk", "topk_fused", "topk_residual_packed"])
def test_packed_entry_point_diagnostics(scan_case, entry, with_ids):
    import torchpq_amd.kernels as K
    from torchpq_amd import _lib
    g = scan_case["g"]
    scan = K.IVFPQTopkHip(m=M)
    assert scan.record_events is None and scan.last_n_split is None and scan.last_call is None
    plain = _call(scan, entry, g, with_ids)
    assert len(plain) == (3 if with_ids else 2)
    ev, ea = scan_case["expect"][entry]
    assert np.array_equal(N(plain[0]), ev) and np.array_equal(N(plain[1]), ea)
    if with_ids:
        assert np.array_equal(N(plain[2]), orc.get_id_by_address(scan_case["a2i"], ea))
    # last_n_split / last_call / last_route
    assert isinstance(scan.last_n_split, int) and scan.last_n_split >= 1
    assert scan.last_call["n_split"] == scan.last_n_split and scan.last_call["n_query"] == NQ
    assert scan.last_route() == scan.route(**scan.last_call) and scan.last_route() in scan.ROUTES.values()
    assert scan.last_workspace is None                      # keep_workspace is off by default
    # one call, one event pair, recorded around it; the outputs do not depend on it
    scan.record_events = []
    timed = _call(scan, entry, g, with_ids)
    assert len(scan.record_events) == 1 and len(scan.record_events[0]) == 2
    torch.cuda.synchronize()
    ms = scan.record_events[0][0].elapsed_time(scan.record_events[0][1])
    assert math.isfinite(ms) and ms >= 0
    assert len(timed) == len(plain) and all(torch.equal(a, b) for a, b in zip(timed, plain))
    # a zero-query call: nothing recorded, empty outputs of the right shapes and dtypes
    empty = _call(scan, entry, g, with_ids, nq=0)
    assert len(scan.record_events) == 1
    assert len(empty) == (3 if with_ids else 2)
    assert [tuple(t.shape) for t in empty] == [(0, K_TOP)] * len(empty)
    assert [t.dtype for t in empty] == [torch.float32, torch.int64, torch.int64][:len(empty)]
    scan.record_events = None
    # keep_workspace
    scan.keep_workspace = True
    kept = _call(scan, entry, g, with_ids)
    ws = scan.last_workspace
    need = _lib.load().tpq_ivfpq_scan_workspace_bytes(NQ, K_TOP, scan.last_n_split, M)
    assert ws is not None and ws.dtype == torch.uint8 and ws.dim() == 1 and ws.numel() >= need
    assert all(torch.equal(a, b) for a, b in zip(kept, plain))
    scan.keep_workspace = False
    _call(scan, entry, g, with_ids)
    assert scan.last_workspace is ws


def _ivf_index(kind):
    from torchpq_amd.index import IVFFlatIndex, IVFPQIndex, IVFPQRIndex
    d, n_cells = 16, 8
    if kind == "ivfpq":
        return IVFPQIndex(d_vector=d, n_subvectors=8, n_cells=n_cells, initial_size=64, device=DEV)
    if kind == "ivfpqr":
        return IVFPQRIndex(d_vector=d, n_subvectors=8, n_subvectors_rerank=8, n_cells=n_cells, initial_size=64,
                           device=DEV)
    return IVFFlatIndex(d_vector=d, n_cells=n_cells, initial_size=64, device=DEV)


@pytest.mark.parametrize("kind", ["ivfpq", "ivfpqr", "ivfflat"])
def test_max_query_batch_split_equals_one_batch(kind):
    """150 queries in batches of 64 (three batches, the last one partial) == the same search in one batch, bit for bit"""
    base, queries = _clustered(5, 16, 2000, 150)
    np.random.seed(5)
    idx = _ivf_index(kind)
    idx.train(T(base))
    idx.add(T(base))
    idx.n_probe = 4
    whole = idx.search(T(queries), k=10, return_address=True)
    assert len(whole) == (2 if kind == "ivfpq" else 3)        # IVFPQIndex.search ignores return_address
    assert (whole[1] >= 0).all()
    idx.max_query_batch = 64
    split = idx.search(T(queries), k=10, return_address=True)
    assert len(split) == len(whole)
    for a, b in zip(whole, split):
        assert a.shape == (150, 10) and a.dtype == b.dtype and torch.equal(a, b)
    two = idx.search(T(queries), k=10)
    assert len(two) == 2 and torch.equal(two[0], whole[0]) and torch.equal(two[1], whole[1])
