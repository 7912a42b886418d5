"""GPU, round 3: the gaps VERDICT r2 named.

* the coarse probe pinned BIT-EXACTLY (sims, cells, probe counts) against oracle.coarse_sims -- every
  kernel of tpq_ivfpq_coarse_probe, tie-laden codebooks included (torchpq/metric.py:75-98,
  index/IVFPQIndex.py:485-512);
* configs[2] (GIST: d=960, m=120, d_sub=8) through the INDEX: train / add / search against the
  oracle -- the non-fused LUT + 16-wave-workgroup + n_split path end to end
  (torchpq/index/IVFPQIndex.py:452-461);
* NaN / Inf queries and LUT entries: no hang, no out-of-range id, padded output;
* train / add / search under torch.inference_mode() (`_version` of inference tensors).
"""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import ivfpq_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def K():
    import torchpq_amd.kernels as k
    from torchpq_amd import _lib
    _lib.load()
    return k


# ---------------------------------------------------------------------------------------------
# coarse probe, bit for bit
# ---------------------------------------------------------------------------------------------
def _probe_data(kind, d, nq, n_cells, rng):
    if kind == "gauss":
        x = (rng.standard_normal((d, nq)) * 20).astype(np.float32)
        c = (rng.standard_normal((d, n_cells)) * 20).astype(np.float32)
    elif kind == "sift":   # small non-negative integers: every product and partial sum is exact
        x = rng.integers(0, 200, (d, nq)).astype(np.float32)
        c = rng.integers(0, 200, (d, n_cells)).astype(np.float32)
    else:                  # "ties": every centroid appears 2-4 times -> exact value ties in every row
        base = rng.integers(0, 50, (d, max(1, n_cells // 3))).astype(np.float32)
        c = base[:, rng.integers(0, base.shape[1], n_cells)]
        x = rng.integers(0, 50, (d, nq)).astype(np.float32)
    return x, c


@pytest.mark.parametrize("kind", ["gauss", "sift", "ties"])
@pytest.mark.parametrize("d,nq,n_cells,n_probe,smart", [
    (128, 777, 1024, 32, True),      # 64 x 256 small-problem tiles
    (32, 5, 16, 16, False),          # 64 x 64 tiles, n_probe == n_cells
    (960, 70, 300, 64, True),        # GIST dimension, ragged cells
    (7, 1, 40, 1, True),             # one query, n_probe 1
    (128, 130, 2000, 200, True),     # long rows, R = 4 selector
    (32, 1100, 16500, 8, True),      # 128-query blocks + group filter (IVF16384 regime)
    (24, 1300, 8200, 64, False),
    (128, 10000, 1024, 32, False),   # configs[1]'s coarse step
    (128, 700, 4096, 16, True),      # the reference grid's IVF4096
    (128, 300, 16384, 128, False),   # ... and IVF16384 at its largest n_probe
    (100, 513, 2052, 40, True),      # ragged everywhere: d, queries, cells (a multiple of 4 only)
    (64, 1000, 3000, 1000, False),   # n_probe close to the candidate list's limit
    (64, 500, 12320, 24, True),      # fp16 route: group maxima of 64 cells, the last group half full
    (32, 400, 17440, 40, False),     # ... of 128 cells, the last group a quarter full
    (48, 300, 4128, 64, True),       # ... of 32 cells, 2 n_probe = the number of groups - 1: the direct list's edge
    (16, 3, 1024, 600, True),        # one-block kernel at R = 16; smart probing on 10 registers per lane
    (8, 2, 512, 300, False),         # ... at R = 8
    (8, 1100, 16500, 100, True),     # group filter (9 query groups x 65 chunks) with an R = 2 selector
])
@pytest.mark.parametrize("route", ["auto", "fp32", "fp16"])
def test_coarse_probe_is_bit_exact(K, kind, d, nq, n_cells, n_probe, smart, route):
    """sims == oracle.coarse_sims gathered at the chosen cells, cells == the (value desc, column asc)
    top-n_probe of the oracle's sims, n_probe_list == smart probing of those sims -- on every route: the fp32-MFMA
    kernels, and the fp16 selection pass + exact candidates (use_tensor_core=True; "auto" takes it from 2 048 cells)"""
    rng = np.random.default_rng(1000 * d + nq + len(kind))
    x, c = _probe_data(kind, d, nq, n_cells, rng)
    sizes = rng.integers(0, 500, n_cells).astype(np.int64)
    start = (np.cumsum(sizes + 3) - sizes - 3).astype(np.int64)
    tc = T(c)
    # (the codebook's share of the fp16 pass prepared once, as IVFPQIndex does -- or per call, inside the workspace)
    prepared = K.CoarseProbeHip.prepare(tc) if (route == "fp16" and nq % 2 == 0) else None
    sims, cells, cs, sz, npl = K.CoarseProbeHip(route=route)(T(x), tc, T(start), T(sizes), n_probe,
                                                             30.0 if smart else None, prepared=prepared)
    full = c_oracle.coarse_sims(x, c)
    ev, ei = orc.topk_desc(full, n_probe)          # value desc, ties -> smaller column
    assert np.array_equal(N(sims), ev)
    assert np.array_equal(N(cells), ei)
    assert np.array_equal(N(cs), start[ei]) and np.array_equal(N(sz), sizes[ei])
    if kind == "ties" and n_probe > 1:
        assert (np.diff(ev, axis=1) == 0).any()    # the case really has ties inside the top-n_probe
    if smart and n_probe > 1:
        exp = orc.smart_probing(ev, n_probe, 30.0)
        got = N(npl)
        # ceil() of an fp32 entropy: exp/log2 may differ in the last ulp between libm and the device;
        # a row sitting on an integer may move by one
        assert np.abs(got - exp).max() <= 1 and (got != exp).mean() < 0.005
        assert np.array_equal(got, N(K.SmartProbingHip()(T(ev), 30.0)))
    else:
        assert np.array_equal(N(npl), np.full(nq, n_probe))


@pytest.mark.parametrize("n_probe", [8, 32])   # 8: the direct candidate list (2 k <= 32 groups); 32: the selector path
@pytest.mark.parametrize("case", ["identical_cells", "nan_query", "huge_centroid", "tiny", "offset", "far_queries",
                                  "near_ties", "mixed_norms"])
def test_coarse_probe_fp16_route_on_degenerate_data(K, case, n_probe):
    """the fp16 selection's exits: a candidate band that overflows its list (thousands of identical centroids: the
    direct list overflows into the selector path, whose list overflows into the exact evaluation of every cell),
    queries / centroids the fp16 scale cannot hold (band = inf), magnitudes of 1e-18, a large common offset --
    the result is the fp32 route's, bit for bit"""
    rng = np.random.default_rng(len(case))
    d, nq, n_cells = 64, 400, 4096
    x = (rng.standard_normal((d, nq)) * 3).astype(np.float32)
    c = (rng.standard_normal((d, n_cells)) * 3).astype(np.float32)
    if case == "identical_cells":
        c[:, 100:3000] = c[:, 100:101]
    elif case == "nan_query":
        x[3, 7] = np.nan
        x[5, 9] = np.inf
    elif case == "huge_centroid":
        c[:, 77] = 1.0e9
    elif case == "tiny":
        x *= 1e-18
        c *= 1e-18
    elif case == "offset":
        x += 1.0e4
        c += 1.0e4
    elif case == "far_queries":      # beyond the range the centroids give the fp16 scale: those queries go exact
        x[:, ::7] *= 50.0
    elif case == "near_ties":        # clusters of centroids closer than the fp16 rounding of the stored fast values
        base = c[:, :n_cells // 4]
        c = (np.repeat(base, 4, axis=1) * (1.0 + 2e-4 * rng.standard_normal((d, n_cells)))).astype(np.float32)
    elif case == "mixed_norms":      # every query has its own power-of-two scale for the stored values
        x *= np.exp2(rng.integers(-6, 3, nq)).astype(np.float32)[None, :]
    z = np.zeros(n_cells, np.int64)
    want = K.CoarseProbeHip(route="fp32")(T(x), T(c), T(z), T(z), n_probe, 30.0)
    tc = T(c)
    got = K.CoarseProbeHip(route="fp16")(T(x), tc, T(z), T(z), n_probe, 30.0, prepared=K.CoarseProbeHip.prepare(tc))
    ok_rows = np.ones(nq, bool)
    if case == "nan_query":
        ok_rows[[7, 9]] = False    # rows of NaN similarities have no defined order on either route
    for a, b in zip(want, got):
        assert np.array_equal(N(a)[ok_rows], N(b)[ok_rows], equal_nan=True)


def test_a_sim_does_not_depend_on_the_batch_it_arrives_in(K):
    """the three coarse kernels (64 x 64, 64 x 256, 128-query blocks) share one arithmetic: a
    query's row is the same bits alone, in a small batch and in a large one"""
    rng = np.random.default_rng(5)
    d, n_cells, n_probe = 96, 1024, 24
    x = (rng.standard_normal((d, 6000)) * 3).astype(np.float32)
    c = (rng.standard_normal((d, n_cells)) * 3).astype(np.float32)
    z = np.zeros(n_cells, np.int64)
    rows = {}
    for nq in (1, 40, 700, 6000):
        s, ce, *_ = K.CoarseProbeHip()(T(x[:, :nq]), T(c), T(z), T(z), n_probe, None)
        rows[nq] = (N(s)[0], N(ce)[0])
    for nq in (40, 700, 6000):
        assert np.array_equal(rows[nq][0], rows[1][0]) and np.array_equal(rows[nq][1], rows[1][1])


# ---------------------------------------------------------------------------------------------
# configs[2] through the index
# ---------------------------------------------------------------------------------------------
def _oracle_search(idx, x, k):
    """oracle search with the oracle's OWN coarse step (bit-exact sims -> cells) and LUT"""
    full = c_oracle.coarse_sims(x, N(idx.vq_codec.codebook))
    _, cells = orc.topk_desc(full, idx.n_probe)
    npl = np.full(x.shape[1], idx.n_probe, np.int64)
    lut = c_oracle.adc_lut(x, N(idx.pq_codec.codebook), idx.distance)
    cs, sz = N(idx._cell_start)[cells], N(idx._cell_size)[cells]
    v, a = c_oracle.scan_topk(N(idx._storage), lut, N(idx._is_empty), cs, sz, npl, k)
    return v, orc.get_id_by_address(N(idx._address2id), a), cells


def test_c3_index_round_trip():
    """BASELINE.json configs[2]'s shape through train / add / search: d=960, m=120 (d_sub=8: the LUT
    is built by adc_lut_kernel, not in the scan workgroup), n_probe=64, k=100, 1 000 queries, then 100 and 10 (the
    scan then splits every query over several workgroups), scan layout and reference layout; values and
    ids equal the oracle's on a query sample, cells equal the oracle's coarse step on every query."""
    from torchpq_amd.index import IVFPQIndex
    d, m, n_cells, n, nq, k = 960, 120, 1024, 200_000, 1000, 100
    g = torch.Generator(device=DEV)
    g.manual_seed(77)
    centers = torch.rand(d, 300, generator=g, device=DEV)

    def sample(count):
        a = torch.randint(0, 300, (count,), generator=g, device=DEV)
        return (centers[:, a] * 0.6 + torch.randn(d, count, generator=g, device=DEV) * 0.08).clamp_(0, 1)

    np.random.seed(77)
    idx = IVFPQIndex(d_vector=d, n_subvectors=m, n_cells=n_cells, initial_size=2 * n // n_cells, device=DEV)
    idx.train(sample(60_000))
    base = sample(n)
    idx.add(base)
    assert idx.n_items == n
    idx.n_probe, idx.use_smart_probing = 64, False
    assert idx.d_subvector == 8 and idx.d_subvector > idx.fused_lut_max_subvector   # the LUT-kernel path
    xq = sample(nq)
    x = N(xq)
    # stored cells / codes are the oracle's: coarse assign and PQ encode of the added vectors
    smp = np.arange(0, n, 997)
    _, lab = c_oracle.max_sim(N(base[:, smp])[None], N(idx.vq_codec.codebook)[None], "euclidean", "expanded")
    adr = N(idx.get_address_by_id(T(smp.astype(np.int64))))
    got_cell = N(idx.get_cell_by_address(T(adr)))
    assert np.array_equal(got_cell, lab[0])
    sel = np.arange(0, nq, 40)
    ev, ei, ecells = _oracle_search(idx, x, k)
    _, cells, _ = idx.probe(xq)
    assert np.array_equal(N(cells), ecells)
    results = {}
    for packed in (True, False):
        idx.use_packed_layout = packed
        v, i = idx.search(xq, k=k)
        results[packed] = (v, i)
        assert np.array_equal(N(v)[sel], ev[sel]) and np.array_equal(N(i)[sel], ei[sel])
    assert torch.equal(results[True][0], results[False][0]) and torch.equal(results[True][1], results[False][1])
    # small batches split every query over several workgroups (n_split > 1): same rows
    scan = idx._ivfpq_topk._scan
    assert scan.last_n_split == 1
    for nb in (100, 10):
        vb, ib = idx.search(xq[:, :nb].contiguous(), k=k)
        assert scan.last_n_split > 1, (nb, scan.last_n_split)
        assert torch.equal(vb, results[True][0][:nb]) and torch.equal(ib, results[True][1][:nb])


# ---------------------------------------------------------------------------------------------
# non-finite inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("packed", [True, False])
@pytest.mark.parametrize("fused", [True, False])
def test_nan_and_inf_queries_do_not_hang_or_leave_the_index(packed, fused, fx_m16):
    """A NaN / Inf query poisons its own LUT (and, through max|LUT|, the packed scan's error bound):
    the call must still return, ids must be stored ids or -1, values of the finite queries must be
    untouched.  The reference returns garbage rows for such queries too; it must not be worse."""
    from torchpq_amd.index import IVFPQIndex
    idx = IVFPQIndex(d_vector=int(fx_m16["d"]), n_subvectors=int(fx_m16["m"]), n_cells=int(fx_m16["n_cells"]),
                     device=DEV)
    idx.load_state_dict({k[3:]: torch.from_numpy(v.copy()) for k, v in fx_m16.items() if k.startswith("sd.")})
    idx.n_probe = int(fx_m16["n_probe"])
    idx.use_packed_layout = packed
    idx.use_fused_lut = fused
    x = fx_m16["queries"].copy()
    nq = x.shape[1]
    assert nq >= 8
    clean_v, clean_i = idx.search(T(x), k=10)
    bad = x.copy()
    bad[0, 1] = np.nan
    bad[:, 3] = np.nan
    bad[5, 4] = np.inf
    bad[2, 6] = -np.inf
    bad[:, 7] = 3.0e38       # finite, but every square overflows
    v, i = idx.search(T(bad), k=10)
    torch.cuda.synchronize()
    v, i = N(v), N(i)
    n_items = idx.n_items
    assert i.shape == (nq, 10) and ((i >= -1) & (i < n_items)).all()
    good = np.setdiff1d(np.arange(nq), [1, 3, 4, 6, 7])
    assert np.array_equal(v[good], N(clean_v)[good]) and np.array_equal(i[good], N(clean_i)[good])
    for q in (1, 3, 4, 6, 7):          # a poisoned row: ids distinct where they are ids
        row = i[q][i[q] >= 0]
        assert len(set(row.tolist())) == len(row)


@pytest.mark.parametrize("layout", ["ref", "packed"])
def test_nan_and_inf_lut_entries_at_the_scan_boundary(K, layout):
    """tpq_ivfpq_scan_topk[_packed] with a caller-supplied LUT that holds NaN, +Inf and -Inf: returns,
    addresses inside the probed cells or -1, finite queries bit-equal to the oracle."""
    rng = np.random.default_rng(9)
    m, n_cells, nq, n_probe, k = 16, 32, 12, 6, 20
    sizes = rng.integers(20, 200, n_cells).astype(np.int64)
    start = (np.cumsum(sizes + 5) - sizes - 5).astype(np.int64)
    n_slots = int(start[-1] + sizes[-1] + 5)
    storage = rng.integers(0, 256, (m // 4, n_slots, 4)).astype(np.uint8)
    lut = (rng.standard_normal((m, nq, 256)) * 10).astype(np.float32)
    lut[3, 0, :] = np.nan
    lut[5, 1, 7] = np.nan
    lut[2, 2, :] = np.inf
    lut[2, 3, 100] = -np.inf
    lut[:, 4, :] = -np.inf
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    npl = np.full(nq, n_probe, np.int64)
    scan = K.IVFPQTopkHip(m=m)
    st = T(storage)
    packed = K.PackCodesHip()(st) if layout == "packed" else None
    v, a = scan.topk(st, T(lut), None, T(start[cells]), T(sizes[cells]), T(npl), n_candidates=k, packed=packed)
    torch.cuda.synchronize()
    v, a = N(v), N(a)
    lo, hi = start[cells][:, None, :], (start[cells] + sizes[cells])[:, None, :]
    inside = ((a[:, :, None] >= lo) & (a[:, :, None] < hi)).any(-1)
    assert (inside | (a == -1)).all()
    ev, ea = c_oracle.scan_topk(storage, lut, None, start[cells], sizes[cells], npl, k)
    fin = np.arange(5, nq)
    assert np.array_equal(v[fin], ev[fin]) and np.array_equal(a[fin], ea[fin])
    # -inf everywhere: nothing beats the (-inf, -1) padding
    assert (a[4] == -1).all() or np.isneginf(v[4]).all()


# ---------------------------------------------------------------------------------------------
# inference mode
# ---------------------------------------------------------------------------------------------
def test_train_add_search_under_inference_mode():
    """tensors made under torch.inference_mode() carry no version counter: is_trained, the graphed
    search snapshot and everything behind them must not read `._version` on them."""
    from torchpq_amd.index import IVFPQIndex
    rng = np.random.default_rng(3)
    d, n = 32, 6000
    base = (rng.standard_normal((d, n)) * 4).astype(np.float32)
    np.random.seed(3)
    with torch.inference_mode():
        idx = IVFPQIndex(d_vector=d, n_subvectors=8, n_cells=16, initial_size=64, device=DEV)
        idx.train(T(base))
        idx.add(T(base[:, :4000]))
        idx.n_probe = 4
        v0, i0 = idx.search(T(base[:, :50]), k=5)
        idx.add(T(base[:, 4000:]))       # grows the buffers inside inference mode
        v1, i1 = idx.search(T(base[:, :50]), k=5)
        assert idx.vq_codec.is_trained and idx.pq_codec.is_trained
        gs = idx.graphed_search(50, k=5)
        gv, gi = gs(T(base[:, :50]))
        assert torch.equal(gv, v1) and torch.equal(gi, i1)
    # ... and the index keeps working outside of it
    assert idx.pq_codec.is_trained
    v2, i2 = idx.search(T(base[:, :50]), k=5)
    assert torch.equal(v1, v2) and torch.equal(i1, i2)
    assert gs.stale_reason() is None
    assert float((i2[:, 0].cpu() == torch.arange(50)).float().mean()) > 0.8


# ---------------------------------------------------------------------------------------------
# ADVICE r2 lows
# ---------------------------------------------------------------------------------------------
def test_remove_by_address_on_holes_with_duplicate_ids(fx_tomb):
    """remove(address=...) on a container with tombstones inside cells AND duplicate ids: the
    addresses are carried through the compaction by its own old -> new map, not through the ids
    (get_address_by_id resolves a duplicated id to ONE address: the wrong slot, or fewer slots,
    were removed before)."""
    from torchpq_amd.index import IVFPQIndex
    fx = fx_tomb
    idx = IVFPQIndex(d_vector=int(fx["d"]), n_subvectors=int(fx["m"]), n_cells=int(fx["n_cells"]), device=DEV)
    idx.load_state_dict({k[3:]: torch.from_numpy(v.copy()) for k, v in fx.items() if k.startswith("sd.")})
    assert idx._has_holes
    a2i = N(idx._address2id)
    live = np.nonzero(a2i >= 0)[0]
    # make every live slot share its id with another one (ids 0..n/2-1, each twice)
    dup = np.arange(live.shape[0]) // 2
    idx._address2id[T(live)] = T(dup.astype(np.int64))
    idx._drop_inverse_id_mapping()
    codes = N(idx._storage).transpose(1, 0, 2).reshape(a2i.shape[0], -1)   # [slot][m]
    victims = live[3::5]                                                   # one of each pair, mostly
    keep = np.setdiff1d(live, victims)
    want = sorted((int(dup[np.searchsorted(live, a)]), codes[a].tobytes()) for a in keep)
    idx.remove(address=T(victims.astype(np.int64)))
    assert not idx._has_holes and idx.n_items == keep.shape[0]
    a2i2 = N(idx._address2id)
    codes2 = N(idx._storage).transpose(1, 0, 2).reshape(a2i2.shape[0], -1)
    got = sorted((int(a2i2[a]), codes2[a].tobytes()) for a in np.nonzero(a2i2 >= 0)[0])
    assert got == want                       # exactly the survivors, each with its own code
    st, sz = N(idx._cell_start), N(idx._cell_size)
    ie = N(idx._is_empty)
    for c in range(idx.n_cells):
        assert np.all(ie[st[c]:st[c] + sz[c]] == 0)


def test_assign_precision_fp32_opts_out_of_the_selection_kernels(monkeypatch):
    """assign_precision="fp32": KMeans.predict (the coarse assign of add) and PQCodec.encode call
    tpq_max_sim only; the default routes the same shapes through the selection kernels -- with the
    same labels."""
    import torchpq_amd.kernels as K
    from torchpq_amd.clustering import KMeans
    from torchpq_amd.codec import PQCodec
    calls = []
    for cls in (K.CoarseAssignHip, K.MaxSimSelectHip):
        orig = cls.__call__
        monkeypatch.setattr(cls, "__call__", (lambda o: lambda self, *a, **kw: (calls.append(type(self).__name__),
                                                                                 o(self, *a, **kw))[1])(orig))
    g = torch.Generator(device=DEV)
    g.manual_seed(11)
    x = torch.randn(64, 300_000, generator=g, device=DEV)
    cent = x[:, :1024].contiguous()
    labels = {}
    for prec in ("bf16x3", "fp32"):
        km = KMeans(n_clusters=1024, assign_precision=prec)
        km.register_buffer("centroids", cent)
        calls.clear()
        labels[prec] = km.predict(x)
        assert ("CoarseAssignHip" in calls) == (prec == "bf16x3"), (prec, calls)
    assert torch.equal(labels["bf16x3"], labels["fp32"])
    codes = {}
    np.random.seed(0)
    for prec in ("bf16x3", "fp32"):
        pq = PQCodec(d_vector=64, n_subvectors=4).to(DEV)          # d_sub = 16 >= split_min_d
        pq.kmeans.assign_precision = prec
        pq.kmeans.register_buffer("centroids", x[:, :256].reshape(4, 16, 256).contiguous())
        pq._trained(True)
        calls.clear()
        codes[prec] = pq.encode(x)
        assert ("MaxSimSelectHip" in calls) == (prec == "bf16x3"), (prec, calls)
    assert torch.equal(codes["bf16x3"], codes["fp32"])


# ---------------------------------------------------------------------------------------------
# fused finish of the packed scan (scan_packed_kernel RM > 0): one launch, the last workgroup of a query
# writes it; tickets from the library's ring
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,k,n_split", [(64, 100, 16), (16, 10, 7), (8, 120, 3), (128, 100, 5), (32, 248, 2)])
def test_fused_finish_over_many_calls_and_two_streams(K, m, k, n_split):
    """a query split over n_split workgroups is finished by the last of them: many back-to-back calls on two
    streams at once (fresh ticket stretches, reset by the finisher) all return the oracle's result"""
    from test_gpu_kernels import _random_index
    rng = np.random.default_rng(m * 131 + k)
    n_cells, nq, n_probe = 40, 9, 12
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 400)
    scan = K.IVFPQTopkHip(m=m)
    st = T(storage)
    packed = K.PackCodesHip()(st)
    cases = []
    for _ in range(3):
        lut = (rng.standard_normal((m, nq, 256)) * 100).astype(np.float32)
        cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
        npl = np.full(nq, n_probe, np.int64)
        cs, sz = start[cells], sizes[cells]
        ev, ea = c_oracle.scan_topk(storage, lut, is_empty, cs, sz, npl, k)
        cases.append((T(lut), T(cs), T(sz), T(npl), ev, ea))
    emp = T(is_empty)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    torch.cuda.synchronize()
    for it in range(40):
        lut, cs, sz, npl, ev, ea = cases[it % 3]
        with torch.cuda.stream(streams[it % 2]):
            v, a = scan.topk(st, lut, emp, cs, sz, npl, n_candidates=k, packed=packed, n_split=n_split)
        outs.append((v, a, ev, ea))
    torch.cuda.synchronize()
    for v, a, ev, ea in outs:
        assert np.array_equal(N(v), ev) and np.array_equal(N(a), ea)


def test_graphed_search_replays_with_its_own_tickets():
    """GraphedSearch captures the two-launch search; replays interleaved with eager calls (which draw other
    ticket stretches) keep returning search()'s result"""
    from torchpq_amd.index import IVFPQIndex
    rng = np.random.default_rng(3)
    d, n = 64, 20000
    x = T(rng.standard_normal((d, n)).astype(np.float32))
    idx = IVFPQIndex(d_vector=d, n_subvectors=16, n_cells=64, initial_size=512, device=DEV, verbose=0)
    idx.train(x[:, :8000])
    idx.add(x)
    idx.n_probe = 8
    q = T(rng.standard_normal((d, 4)).astype(np.float32))
    ev, ei = idx.search(q, k=10)
    g = idx.graphed_search(4, k=10)
    for _ in range(5):
        gv, gi = g(q)
        v2, i2 = idx.search(q, k=10)
        assert torch.equal(gv, ev) and torch.equal(gi, ei) and torch.equal(v2, ev) and torch.equal(i2, ei)
