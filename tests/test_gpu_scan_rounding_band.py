"""GPU: the packed scan's top-k where the fp32 summation order decides the k-th place.

The packed routes select with a fast sum (another association order; a 16-bit fixed-point table on the large-batch
routes of m = 64) and keep what lies within a band of the running k-th value for the exact ascending-j chain; the band is
2 * delta_rel * sum_j max|LUT_j| (csrc/scan_packed_kernel.h; the residual scan adds |base| + cell_bound[cell]).  Bit-equality
with the oracle therefore rests on band >= |fast - exact|, which zero-mean tables never strain: here the tables carry a
large common offset (tests_support.offset_lut / offset_query_codebook), so that the bound is far above the spread of the
candidates -- test_scan_band_inputs_cpu.py shows, without a kernel, that the order then changes the top-k members.

Every case names its route and checks it, compares values, addresses and ids with the oracle bit for bit, and prints the
number of queries redone exactly; where a regime was seen on the MI355X it is asserted since (tests_support.BAND_CASES:
"held" = orders disagree on the CPU and nothing was redone, "redone" = the band overflowed or the table could not be
scaled and the exact kernel took the query).
"""
import numpy as np
import pytest
import torch

import tests_support as S
from oracle import c_oracle
from oracle import ivfpq_oracle as orc
from tests_support import N, T

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def K():
    import torchpq_amd.kernels as k
    from torchpq_amd import _lib
    _lib.load()
    return k


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _check(got, ev, ea, a2i, tag):
    v, a, i = (N(t) for t in got)
    assert np.array_equal(a, ea), tag
    assert np.array_equal(_bits(v), _bits(ev)), tag
    assert np.array_equal(i, orc.get_id_by_address(a2i, ea)), tag


def _regime(scan, nq, expect, tag):
    redone = scan.last_redone(nq)
    print(f"BAND-GPU {tag} route={scan.last_route()} redone={redone}/{nq}")
    if expect == "held":
        assert redone == 0, tag
    elif expect == "redone":
        assert redone >= 1, tag
    return redone


@pytest.mark.parametrize("case", S.BAND_CASES, ids=[c["id"] for c in S.BAND_CASES])
def test_offset_tables_equal_the_oracle_on_every_route(K, case):
    ix = S.band_case_inputs(case)
    m, k, nq = case["m"], case["k"], case["nq"]
    ev, ea = c_oracle.scan_topk(ix["storage"], ix["lut"], ix["is_empty"], ix["cs"], ix["sz"], ix["npl"], k)
    scan = K.IVFPQTopkHip(m=m)
    scan.keep_workspace = True
    st = T(ix["storage"])
    packed = K.PackCodesHip()(st) if case["packed"] else None
    common = dict(n_candidates=k, packed=packed, address2id=T(ix["a2i"]), n_split=case["n_split"],
                  slots_hint=case["hint"])
    if case["src"] == "lut":
        got = scan.topk(st, T(ix["lut"]), T(ix["is_empty"]), T(ix["cs"]), T(ix["sz"]), T(ix["npl"]), **common)
    else:
        got = scan.topk_fused(st, T(ix["query"]), T(ix["codebook"]), T(ix["is_empty"]), T(ix["cs"]), T(ix["sz"]),
                              T(ix["npl"]), distance=case["distance"], **common)
    torch.cuda.synchronize()
    assert scan.last_route() == case["route"], (case["id"], scan.last_route())
    _check(got, ev, ea, ix["a2i"], case["id"])
    _regime(scan, nq, case["expect"], case["id"])


def test_every_route_is_named_by_a_case(K):
    named = {c["route"] for c in S.BAND_CASES} | {"sorted_lists"}   # (the residual cases below: sorted_lists)
    assert named == set(K.IVFPQTopkHip.ROUTES.values()) - {"rejected"}


# ---------------------------------------------------------------------------------------------
# the edges of the 16-bit route's `scalable` test and of the fp32 large-batch route's bound
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route,m,ds", [("dump_sel16", 64, 1), ("dump_sel16", 64, 2), ("dump_f32", 32, 4)])
def test_tables_at_the_edge_of_what_can_be_scaled(K, route, m, ds):
    """inner-product tables whose bound sum_j max|LUT_j| sits just under 1e37 (every J_j just under 1e37 / m: the query
    stays on the fast path with the largest table it admits) or just over it (the prologue hands the query to the exact
    kernel): both must equal the oracle, and every query over the limit is counted as redone"""
    nq, k, n_probe = 1100, 10, 8
    ix = S.band_index(m * 31 + ds, m, nq, n_probe)
    rng = ix["rng"]
    cb = rng.uniform(-1.0, 1.0, (m, ds, 256)).astype(np.float32)
    q = rng.uniform(0.5, 1.0, (m * ds, nq)).astype(np.float32)
    unit = np.abs(c_oracle.adc_lut(q, cb, "inner")).max(axis=2).astype(np.float64).sum(axis=0)     # [nq]
    over = np.zeros(nq, bool)
    over[[0, 3, 500, 1099]] = True
    over[rng.random(nq) < 0.02] = True
    q = (q.astype(np.float64) * (np.where(over, 1.03e37, 0.97e37) / unit)).astype(np.float32)
    lut = c_oracle.adc_lut(q, cb, "inner")
    bound = np.abs(lut).max(axis=2).astype(np.float64).sum(axis=0)
    assert np.isfinite(lut).all() and (bound[over] > 1.02e37).all() and (bound[~over] < 0.98e37).all()
    assert (bound[~over] > 0.96e37).all() and np.abs(lut).max() < 1e37
    ev, ea = c_oracle.scan_topk(ix["storage"], lut, ix["is_empty"], ix["cs"], ix["sz"], ix["npl"], k)
    assert np.isfinite(ev[ea >= 0]).all()
    scan = K.IVFPQTopkHip(m=m)
    scan.keep_workspace = True
    st = T(ix["storage"])
    got = scan.topk_fused(st, T(q), T(cb), T(ix["is_empty"]), T(ix["cs"]), T(ix["sz"]), T(ix["npl"]), n_candidates=k,
                          distance="inner", packed=K.PackCodesHip()(st), address2id=T(ix["a2i"]), n_split=1)
    torch.cuda.synchronize()
    assert scan.last_route() == route
    _check(got, ev, ea, ix["a2i"], route)
    redone = _regime(scan, nq, None, f"edge-{route}-m{m}-ds{ds}")
    assert redone >= int(over.sum())


# ---------------------------------------------------------------------------------------------
# the residual scan: |base| and cell_bound are part of the bound
# ---------------------------------------------------------------------------------------------
_RES = [(m, k, which, A, fused)
        for m, k in ((8, 10), (16, 300), (64, 100), (128, 100), (32, 1))
        for which in ("base", "part2", "both")
        for A, fused in ((2 ** 14, False), (2 ** 20, True), (2 ** 20, False))] + \
       [(m, k, "none", 0, fused) for m, k, fused in ((8, 10, False), (64, 100, True), (128, 100, False))]


@pytest.mark.parametrize("m,k,which,A,fused", _RES)
def test_residual_scan_with_large_base_sims_and_part2(K, m, k, which, A, fused):
    """tpq_ivfpq_scan_topk_residual_packed with base_sims ~ +-A (|base| dominates the bound), part2 ~ A (cell_bound
    does), or both; part1 given or built in the workgroup; n_split 1 and 3"""
    rng = np.random.default_rng(m * 13 + k + int(np.log2(A or 1)) * 1000 + len(which) + 7 * fused)
    n_cells, nq, n_probe, ds = 40, 37, 8, 2
    from test_gpu_kernels import _random_index
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 150, 20 if m == 64 else 0, 0.0)
    cb = (rng.standard_normal((m, ds, 256)) * 8).astype(np.float32)
    query = (rng.standard_normal((m * ds, nq)) * 8).astype(np.float32)
    part1 = orc.residual_part1(query, cb)
    part2 = (rng.standard_normal((n_cells, m, 256)) * 50).astype(np.float32)
    base = (rng.standard_normal((nq, n_probe)) * 300).astype(np.float32)
    if which in ("part2", "both"):   # a cell-wide offset, its sign by cell
        part2 = (part2 + rng.choice([-1.0, 1.0], (n_cells, 1, 1)) * A).astype(np.float32)
    if which in ("base", "both"):
        base = (base + rng.choice([-1.0, 1.0], (nq, n_probe)) * A).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    cells[3, 1] = cells[3, 0]
    npl = rng.integers(1, n_probe + 1, nq).astype(np.int64)
    npl[:5] = n_probe
    cs, sz = start[cells], sizes[cells]
    ev, ea = c_oracle.scan_topk_residual(storage, part1, part2, cells, base, is_empty, cs, sz, npl, k)
    scan = K.IVFPQTopkHip(m=m)
    scan.keep_workspace = True
    st, p2 = T(storage), T(part2)
    packed = K.PackCodesHip()(st)
    slot_term, cell_bound = K.ResidualSlotTermsHip()(st, p2, T(start), T(sizes))
    np.testing.assert_allclose(N(cell_bound), np.abs(part2).max(-1).sum(-1), rtol=1e-5)
    for n_split in (1, 3):
        got = scan.topk_residual_packed(
            st, packed, p2, slot_term, cell_bound, T(cells), T(base), T(is_empty), T(cs), T(sz), T(npl),
            n_candidates=k, part1=None if fused else T(part1), query=T(query) if fused else None,
            codebook=T(cb) if fused else None, address2id=T(a2i), n_split=n_split)
        torch.cuda.synchronize()
        assert scan.last_route() == "sorted_lists"
        tag = f"residual-m{m}-k{k}-{which}-A{int(np.log2(A or 1))}-{'fused' if fused else 'part1'}-s{n_split}"
        _check(got, ev, ea, a2i, tag)
        _regime(scan, nq, None, tag)


# ---------------------------------------------------------------------------------------------
# index level: un-centred data
# ---------------------------------------------------------------------------------------------
def _uncentred(seed, d, n, nq, offset):
    base, queries = S._clustered(seed, d, n, nq, n_centers=30)
    return (base + np.float32(offset)).astype(np.float32), (queries + np.float32(offset)).astype(np.float32)


@pytest.mark.parametrize("distance,residual", [("euclidean", False), ("cosine", False), ("euclidean", True)])
def test_index_on_uncentred_data(distance, residual):
    """IVFPQIndex (d = 32, m = 8, 16 cells, 6 000 vectors) on vectors that all carry the same large constant -- the cosine
    table's entries (all vectors nearly parallel) and the residual scan's part2 are then far above the spread of the values: search() equals
    the oracle driven by the index's own coarse step; the graphed search and a max_query_batch split equal search()"""
    from test_gpu_index import _expected_search
    from torchpq_amd.index import IVFPQIndex
    d, n, nq, k = 32, 6000, 37, 10
    base, queries = _uncentred(21, d, n, nq, 1000.0)
    np.random.seed(21)
    idx = IVFPQIndex(d_vector=d, n_subvectors=8, n_cells=16, initial_size=512, device=DEV, distance=distance,
                     pq_use_residual=residual)
    idx.train(T(base))
    idx.add(T(base))
    idx.n_probe = 6
    idx.use_smart_probing = False
    assert idx.use_packed_layout
    v, i = idx.search(T(queries), k=k)
    if residual:
        topk_sims, cells, npl = idx.probe(T(queries))
        cells_n = N(cells)
        p1, p2 = idx.precomputed_adc_residual_precomputed(T(queries))
        ev, ea = c_oracle.scan_topk_residual(N(idx._storage), N(p1), N(p2.contiguous()), cells_n, N(topk_sims),
                                             N(idx._is_empty), N(idx._cell_start)[cells_n], N(idx._cell_size)[cells_n],
                                             N(npl), k)
        ei = orc.get_id_by_address(N(idx._address2id), ea)
        # the construction: the tables' entries are far above the values they sum to
        assert min(np.abs(N(p1)).max(), np.abs(N(p2)).max()) > 20 * np.abs(ev[ea >= 0]).max()
    else:   # (cosine: search() normalises the queries, probe() and the oracle's table take them normalised)
        from torchpq_amd import util
        xn = N(util.normalize(T(queries), dim=0)) if distance == "cosine" else queries
        ev, ei, _, _ = _expected_search(idx, xn, k)
    assert np.array_equal(_bits(N(v)), _bits(ev))
    assert np.array_equal(N(i), ei)
    g = idx.graphed_search(nq, k=k)
    gv, gi = g(T(queries))
    assert torch.equal(gv, v) and torch.equal(gi, i)
    idx.max_query_batch = 16   # 37 queries -> 3 batches
    bv, bi = idx.search(T(queries), k=k)
    assert torch.equal(bv, v) and torch.equal(bi, i)
