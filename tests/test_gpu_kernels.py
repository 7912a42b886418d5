"""GPU parity: every C-ABI entry point (through torchpq_amd.kernels) against the oracle.

Bit-exact for integer / byte / index work and for the fp32 values whose summation order the
reference fixes (scan, LUT, max_sim); fp32 tolerance 1e-4 relative (BASELINE.json) elsewhere.
"""
import os

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
    _lib.load()  # fail loudly if libtorchpq_amd.so is missing
    return k


def _sd(fx, key):
    return fx["sd." + key]


# ---------------------------------------------------------------------------------------------
# list scan
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fx_tiny", "fx_m16"])
@pytest.mark.parametrize("layout", ["ref", "packed"])
def test_scan_matches_golden(K, name, layout, request):
    fx = request.getfixturevalue(name)
    m = int(fx["m"])
    scan = K.IVFPQTopkHip(m=m)
    storage = T(_sd(fx, "_storage"))
    packed = K.PackCodesHip()(storage) if layout == "packed" else None
    lut = T(fx["ref_lut"])
    a2i = T(_sd(fx, "_address2id"))
    cs = T(_sd(fx, "_cell_start")[fx["ref_cells"]])
    sz = T(_sd(fx, "_cell_size")[fx["ref_cells"]])
    nq = int(fx["nq"])
    for smart in (0, 1):
        npl = fx["ref_nprobe_list"] if smart else np.full(nq, int(fx["n_probe"]), np.int64)
        for k in fx["ks"]:
            k = int(k)
            for n_split in (1, 3):
                v, a, i = scan.topk(storage, lut, T(_sd(fx, "_is_empty")), cs, sz, T(npl),
                                    n_candidates=k, packed=packed, address2id=a2i, n_split=n_split)
                assert np.array_equal(N(v), fx[f"orc_vals_s{smart}_k{k}"]), (smart, k, n_split)
                assert np.array_equal(N(a), fx[f"orc_addr_s{smart}_k{k}"]), (smart, k, n_split)
                assert np.array_equal(N(i), fx[f"orc_ids_s{smart}_k{k}"]), (smart, k, n_split)


def _random_index(rng, m, n_cells, mean_size, n_tomb=0, dup_frac=0.0, sizes=None):
    """Ragged cells (some empty) with slack, random codes; optional tombstones / duplicate codes.
    `sizes`: the cells' sizes, given instead of drawn."""
    if sizes is None:
        sizes = rng.poisson(mean_size, n_cells).astype(np.int64)
        sizes[rng.random(n_cells) < 0.1] = 0
    sizes = np.asarray(sizes, np.int64)
    caps = sizes + rng.integers(0, 9, n_cells)
    start = np.cumsum(caps) - caps
    cap = int(caps.sum()) + 5
    storage = rng.integers(0, 256, (m // 4, cap, 4), dtype=np.uint8)
    if dup_frac > 0:  # exact ties: copy one code vector over a fraction of the slots
        dup = rng.random(cap) < dup_frac
        storage[:, dup, :] = storage[:, :1, :]
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    if n_tomb:
        occ = np.nonzero(is_empty == 0)[0]
        is_empty[rng.choice(occ, min(n_tomb, occ.size), replace=False)] = 1
    a2i = np.where(is_empty == 0, np.arange(cap) * 7 + 3, -1).astype(np.int64)
    return storage, is_empty, start, sizes, a2i


@pytest.mark.parametrize("m,k,n_probe,n_split,layout,tomb,dup", [
    (8, 1, 4, 1, "ref", 0, 0.0),
    (8, 10, 6, 2, "packed", 40, 0.0),
    (16, 64, 8, 1, "packed", 0, 0.3),
    (16, 100, 8, 5, "ref", 25, 0.2),
    (32, 128, 16, 1, "packed", 0, 0.0),
    (64, 100, 12, 1, "packed", 0, 0.0),
    (64, 100, 12, 4, "ref", 0, 0.05),
    (64, 200, 12, 2, "packed", 17, 0.0),
    (64, 1024, 24, 1, "packed", 0, 0.0),
    (120, 100, 10, 1, "packed", 0, 0.0),
    (120, 33, 10, 3, "ref", 9, 0.0),
    (36, 7, 5, 1, "packed", 0, 0.0),   # m without a scan-layout kernel: reference-layout path
    (12, 300, 9, 2, "ref", 0, 0.1),
    (4, 10, 6, 1, "packed", 5, 0.0),
    (12, 300, 9, 2, "packed", 0, 0.1),
    (20, 50, 7, 1, "packed", 0, 0.0),
    (24, 7, 5, 3, "packed", 0, 0.2),
    (28, 100, 8, 1, "packed", 11, 0.0),
    (40, 64, 8, 2, "packed", 0, 0.0),
    (48, 130, 11, 1, "packed", 0, 0.05),
    (56, 10, 6, 1, "packed", 0, 0.0),
    (96, 100, 10, 2, "packed", 7, 0.0),
    (128, 100, 10, 1, "packed", 0, 0.0),
    (128, 500, 10, 3, "packed", 0, 0.3),
    (64, 510, 12, 1, "packed", 0, 0.0),    # k in (504, 512] at m = 64: the pools of 1 024 entries (with counting rounds)
])
def test_scan_random_vs_oracle(K, m, k, n_probe, n_split, layout, tomb, dup):
    rng = np.random.default_rng(hash((m, k, n_probe, n_split)) % 2**32)
    n_cells, nq = 40, 37
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 150, tomb, dup)
    lut = (rng.standard_normal((m, nq, 256)) * 100).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    cells[3, 1] = cells[3, 0]  # repeated cell right after itself: skipped (ivfpq_topk.cu:864-866)
    npl = rng.integers(0, n_probe + 1, nq).astype(np.int64)
    npl[:5] = n_probe
    cs, sz = start[cells], sizes[cells]
    ev, ea = c_oracle.scan_topk(storage, lut, is_empty, cs, sz, npl, k)
    eid = orc.get_id_by_address(a2i, ea)
    scan = K.IVFPQTopkHip(m=m)
    st = T(storage)
    packed = K.PackCodesHip()(st) if layout == "packed" else None
    v, a, i = scan.topk(st, T(lut), T(is_empty), T(cs), T(sz), T(npl), n_candidates=k,
                        packed=packed, address2id=T(a2i), n_split=n_split)
    assert np.array_equal(N(v), ev)
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(i), eid)
    if tomb == 0:  # no tombstones -> is_empty may be omitted
        v2, a2 = scan.topk(st, T(lut), None, T(cs), T(sz), T(npl), n_candidates=k, packed=packed,
                           n_split=n_split)
        assert np.array_equal(N(v2), ev) and np.array_equal(N(a2), ea)


@pytest.mark.parametrize("m,k,n_probe,mean,tomb,route,nw,tile", [
    (16, 40, 8, 300, 0, "dump_f32", 4, 256),        # cells of 2 tiles: 14 or 16 tiles per workgroup
    (64, 100, 5, 150, 25, "dump_sel16", 4, 64),     # cells of 3 tiles: 12 or 15 tiles per workgroup; tombstones
    (64, 300, 4, 450, 0, "dump_sel16_w8", 8, 64),   # cells of 7 or 8 tiles: 21 .. 32 tiles per workgroup
])
def test_scan_large_batch_routes_vs_oracle(K, m, k, n_probe, mean, tomb, route, nw, tile):
    """The large-batch routes (the scan workgroup ends with its waves' lists of fast values; scan_finish_exact_kernel
    does the rest) against the ORACLE, bit for bit: 1 024 queries (the routes' threshold), the LUT built in the
    workgroups, cells of unequal size -- one empty, none a multiple of the tile (`tile` slots: 64 x slots per lane) --
    and per-query probe counts.  A query that probes all its cells is between 2 NW + 1 and 4 NW + 1 tiles (NW = `nw`
    waves per workgroup, one workgroup per query): the tile pipeline's prologue, steady state and both exits.  The
    shape is asserted, not hoped for."""
    rng = np.random.default_rng(m * 1000 + k)
    n_cells, nq, ds = 40, 1024, 2
    sizes = mean - 20 + (np.arange(n_cells) * 7) % 41
    sizes[sizes % tile == 0] += 1
    sizes[0] = 0
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, mean, tomb, 0.0, sizes=sizes)
    cb = (rng.standard_normal((m, ds, 256)) * 20).astype(np.float32)
    q = (rng.standard_normal((m * ds, nq)) * 20).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    cells[0, 0] = 0 if 0 not in cells[0] else cells[0, 0]  # (query 0 probes the empty cell for sure)
    npl = rng.integers(0, n_probe + 1, nq).astype(np.int64)
    npl[:900] = n_probe
    cs, sz = start[cells], sizes[cells]
    assert (sizes[1:] % tile != 0).all() and len(set(sizes.tolist())) > 10
    tiles = ((sz + tile - 1) // tile)[npl == n_probe].sum(axis=1)
    assert 2 * nw + 1 <= tiles.min() and tiles.max() <= 4 * nw + 1, (tiles.min(), tiles.max())
    ev, ea = c_oracle.scan_topk(storage, c_oracle.adc_lut(q, cb, "euclidean"), is_empty, cs, sz, npl, k)
    scan = K.IVFPQTopkHip(m=m)
    st = T(storage)
    v, a, i = scan.topk_fused(st, T(q), T(cb), T(is_empty) if tomb else None, T(cs), T(sz), T(npl), n_candidates=k,
                              packed=K.PackCodesHip()(st), address2id=T(a2i), n_split=1, slots_hint=n_probe * mean)
    assert scan.last_route() == route
    assert np.array_equal(N(v), ev)
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(i), orc.get_id_by_address(a2i, ea))


@pytest.mark.parametrize("m,k,n_split", [(64, 256, 1), (64, 200, 2), (16, 100, 1), (32, 500, 1)])
def test_scan_short_lists_overflow_is_redone_exactly(K, m, k, n_split):
    """The packed scan sizes its per-wave candidate lists for 2k entries over the workgroup
    (scan_host.h list_regs_scan), counting on the round-robin tile deal to spread the top-k.  Here
    every one of the 1024 best vectors of query 0 sits in a 64-slot block whose tile goes to wave 0
    (blocks 2048 slots apart: tile index = 0 mod 32 for 64-, 128- and 256-slot tiles), so wave 0's list
    overflows with live candidates; the query must be flagged and redone by the exact kernel, and
    the result must still be the oracle's, bit for bit.  (A library built with
    -DTPQ_EXP_NO_OVERFLOW_FLAG fails all four cases: the flag is what makes them pass.)"""
    rng = np.random.default_rng(m * 1000 + k)
    n, nq = 32768, 3
    lut = (rng.standard_normal((m, nq, 256)) * 100).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    best = lut[:, 0, :].argmax(axis=1).astype(np.uint8)
    top = np.nonzero((np.arange(n) // 64) % 32 == 0)[0]
    codes[top] = best
    for t in top:  # distinct scores: two random subvectors keep their random code
        j = rng.choice(m, 2, replace=False)
        codes[t, j] = rng.integers(0, 256, 2)
    storage = np.ascontiguousarray(codes.reshape(n, m // 4, 4).transpose(1, 0, 2))
    is_empty = np.zeros(n, np.uint8)
    cs = np.zeros((nq, 1), np.int64)
    sz = np.full((nq, 1), n, np.int64)
    npl = np.ones(nq, np.int64)
    ev, ea = c_oracle.scan_topk(storage, lut, is_empty, cs, sz, npl, k)
    assert np.isin(ea[0], top).all()  # the construction holds: query 0's answer is inside the blocks
    scan = K.IVFPQTopkHip(m=m)
    st = T(storage)
    scan.keep_workspace = True
    # (slots_hint = one long cell: the kernel then keeps the SHORT lists this test is about; without a hint
    # it sizes them for 4k entries and nothing overflows)
    v, a = scan.topk(st, T(lut), T(is_empty), T(cs), T(sz), T(npl), n_candidates=k,
                     packed=K.PackCodesHip()(st), n_split=n_split, slots_hint=n)
    assert np.array_equal(N(v), ev)
    assert np.array_equal(N(a), ea)
    if k <= 248:  # (one-launch finish: the diagnostics word says the redo ran)
        assert scan.last_redone(nq) >= 1


def test_scan_packed_falls_back_when_lds_is_short(K):
    """m=128 with a 700-entry probe table does not fit 160 KiB next to the 128-KiB LUT: the packed
    entry point must still answer (reference-layout kernel), bit-exactly."""
    rng = np.random.default_rng(77)
    m, n_cells, nq, n_probe, k = 128, 800, 5, 700, 40
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 6)
    lut = (rng.standard_normal((m, nq, 256)) * 100).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    npl = np.full(nq, n_probe, np.int64)
    cs, sz = start[cells], sizes[cells]
    ev, ea = c_oracle.scan_topk(storage, lut, is_empty, cs, sz, npl, k)
    st = T(storage)
    v, a = K.IVFPQTopkHip(m=m).topk(st, T(lut), T(is_empty), T(cs), T(sz), T(npl), n_candidates=k,
                                    packed=K.PackCodesHip()(st), n_split=2)
    assert np.array_equal(N(v), ev) and np.array_equal(N(a), ea)


def test_scan_empty_and_degenerate(K):
    rng = np.random.default_rng(5)
    m = 16
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, 8, 30)
    scan = K.IVFPQTopkHip(m=m)
    lut = T(rng.standard_normal((m, 4, 256)).astype(np.float32))
    cells = np.tile(np.arange(3), (4, 1))
    sz = sizes[cells].copy()
    sz[0] = 0  # query 0 scans nothing
    npl = np.array([3, 0, 3, 1], np.int64)
    v, a = scan.topk(T(storage), lut, T(is_empty), T(start[cells]), T(sz), T(npl), n_candidates=5)
    v, a = N(v), N(a)
    assert np.all(np.isneginf(v[0])) and np.all(a[0] == -1)
    assert np.all(np.isneginf(v[1])) and np.all(a[1] == -1)
    ev, ea = c_oracle.scan_topk(storage, N(lut), is_empty, start[cells], sz, npl, 5)
    assert np.array_equal(v, ev) and np.array_equal(a, ea)
    # zero queries
    v0, a0 = scan.topk(T(storage), lut[:, :0].contiguous(), None, T(start[cells][:0]),
                       T(sz[:0]), T(npl[:0]), n_candidates=5)
    assert v0.shape == (0, 5) and a0.shape == (0, 5)


def test_scan_argument_errors(K):
    from torchpq_amd._lib import TorchPQAmdError, load, ptr
    lib = load()
    x = torch.zeros(16, device=DEV)
    rc = lib.tpq_ivfpq_scan_topk(ptr(x), ptr(x), None, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), None,
                                 None, 10, 1, 1, 6, 5, 1, None, 0, None)  # m % 4 != 0
    assert rc == -1 and b"multiple of 4" in lib.tpq_last_error()
    rc = lib.tpq_ivfpq_scan_topk(ptr(x), ptr(x), None, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), None,
                                 None, 10, 1, 1, 8, 2000, 1, None, 0, None)  # k > 1024
    assert rc == -1
    rc = lib.tpq_ivfpq_scan_topk(ptr(x), ptr(x), None, ptr(x), ptr(x), ptr(x), ptr(x), ptr(x), None,
                                 None, 10, 1, 1, 8, 5, 4, None, 0, None)  # split without workspace
    assert rc == -3
    with pytest.raises(TorchPQAmdError):
        K.IVFPQTopkHip(m=8).topk(torch.zeros(2, 4, 4, dtype=torch.uint8), torch.zeros(8, 1, 256),
                                 None, torch.zeros(1, 1, dtype=torch.long),
                                 torch.zeros(1, 1, dtype=torch.long),
                                 torch.zeros(1, dtype=torch.long), n_candidates=1)  # CPU tensors


def test_pack_is_a_per_slot_permutation(K):
    rng = np.random.default_rng(9)
    for m in (8, 16, 24, 64, 120):
        storage = rng.integers(0, 256, (m // 4, 300, 4), dtype=np.uint8)
        packed = N(K.PackCodesHip()(T(storage)))
        w = packed.shape[2]
        codes = storage.transpose(0, 2, 1).reshape(m, 300)         # [m, slot]
        pk = packed.transpose(0, 2, 1).reshape(m, 300)             # [position, slot]
        assert np.array_equal(np.sort(codes, axis=0), np.sort(pk, axis=0))
        assert w == (16 if m % 16 == 0 else 8 if m % 8 == 0 else 4)


# ---------------------------------------------------------------------------------------------
# LUT, select, smart probing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,ds,nq", [(8, 4, 16), (64, 2, 100), (120, 8, 33), (16, 1, 5), (4, 7, 70)])
@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_adc_lut_bit_exact_vs_c_oracle(K, m, ds, nq, distance):
    rng = np.random.default_rng(m * 100 + ds)
    cb = (rng.standard_normal((m, ds, 256)) * 30).astype(np.float32)
    q = (rng.standard_normal((m * ds, nq)) * 30).astype(np.float32)
    got = N(K.AdcLutHip()(T(q), T(cb), distance))
    exp = c_oracle.adc_lut(q, cb, distance)
    assert np.array_equal(got, exp)
    ref_formula = orc.adc_lut(q, cb, distance)  # reference formula, BLAS summation order
    np.testing.assert_allclose(got, ref_formula, rtol=1e-4, atol=1e-4 * np.abs(ref_formula).max())


def test_adc_lut_matches_reference_golden(K, fx_tiny, fx_m16):
    for fx in (fx_tiny, fx_m16):
        got = N(K.AdcLutHip()(T(fx["queries"]), T(_sd(fx, "pq_codec.kmeans.centroids"))))
        ref = fx["ref_lut"]
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=1e-6 * np.abs(ref).max())


@pytest.mark.parametrize("rows,cols,k", [(5, 7, 1), (33, 1024, 32), (10, 300, 64), (9, 1000, 100),
                                         (4, 16384, 64), (3, 70, 70), (2, 5000, 1024), (17, 64, 8)])
def test_topk_select_exact(K, rows, cols, k):
    rng = np.random.default_rng(rows * cols + k)
    x = rng.standard_normal((rows, cols)).astype(np.float32)
    x[:, ::3] = np.round(x[:, ::3], 1)  # plenty of exact ties
    v, i = K.TopkSelectHip()(T(x), k=k)
    ev, ei = orc.topk_desc(x, k)
    assert np.array_equal(N(v), ev)
    assert np.array_equal(N(i), ei)


def test_topk_select_matches_reference_golden(K, fx_m16):
    v, i = K.TopkSelectHip()(T(fx_m16["ref_sims"]), k=int(fx_m16["n_probe"]))
    assert np.array_equal(N(v), fx_m16["ref_topk_sims"])
    assert np.array_equal(N(i), fx_m16["ref_cells"])  # no ties in this fixture


def test_smart_probing(K, fx_tiny, fx_m16):
    for fx in (fx_tiny, fx_m16):
        got = N(K.SmartProbingHip()(T(fx["ref_topk_sims"]), 30.0))
        assert np.array_equal(got, fx["ref_nprobe_list"])
    rng = np.random.default_rng(0)
    s = -np.abs(rng.standard_normal((500, 32)).astype(np.float32)) * 5e4
    s = -np.sort(-s, axis=1)
    got = N(K.SmartProbingHip()(T(s), 30.0))
    exp = orc.smart_probing(s, 32, 30.0)
    # ceil() of an fp32 entropy: a last-ulp difference in exp/log2 can flip a value sitting
    # exactly on an integer; allow |diff| <= 1 on < 0.5 % of the rows
    assert np.abs(got - exp).max() <= 1 and (got != exp).mean() < 0.005
    assert got.min() >= 1 and got.max() <= 32


# ---------------------------------------------------------------------------------------------
# k-means kernels
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("l,d,m,n", [(1, 128, 300, 64), (3, 2, 1000, 256), (2, 8, 257, 256),
                                     (1, 33, 129, 300), (4, 7, 64, 5), (1, 64, 500, 1024)])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_max_sim_bit_exact_vs_c_oracle(K, l, d, m, n, distance):
    rng = np.random.default_rng(l * 1000 + d * 10 + n)
    A = (rng.standard_normal((l, d, m)) * 10).astype(np.float32)
    B = (rng.standard_normal((l, d, n)) * 10).astype(np.float32)
    B[:, :, n // 2] = B[:, :, 0]  # duplicate centroid: tie -> smallest index
    v, i = K.MaxSimHip(distance=distance)(T(A), T(B), dim=2, mode="tn")
    ev, ei = c_oracle.max_sim(A, B, distance, "expanded")
    assert np.array_equal(N(i), ei)
    assert np.array_equal(N(v), ev)
    if l == 1:  # 2-D call form used by KMeans
        v2, i2 = K.MaxSimHip(distance=distance)(T(A[0]), T(B[0]), dim=1, mode="tn")
        assert np.array_equal(N(i2), ei[0]) and np.array_equal(N(v2), ev[0])


def _max_sim_f64(A, B, distance):
    """float64 similarities [l, m, n] and their scale sum|a_k b_k| (+ norms): the yardstick both
    assign kernels are held to"""
    a, b = A.astype(np.float64), B.astype(np.float64)
    dots = np.einsum("ldm,ldn->lmn", a, b)
    absd = np.einsum("ldm,ldn->lmn", np.abs(a), np.abs(b))
    if distance == "euclidean":
        a2, b2 = (a * a).sum(1)[:, :, None], (b * b).sum(1)[:, None, :]
        return 2 * dots - a2 - b2, 2 * absd + a2 + b2
    return dots, absd


@pytest.mark.parametrize("l,d,m,n,scale", [(2, 64, 3000, 256, 10.0), (1, 17, 1000, 200, 1e3),
                                           (3, 33, 777, 300, 1e-3), (1, 12, 5000, 37, 1.0),
                                           (1, 48, 300, 600, 10.0), (2, 64, 40, 256, 1.0),
                                           (1, 1, 500, 9, 1.0)])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_max_sim_split_has_fp32_accuracy(K, l, d, m, n, scale, distance):
    """tpq_max_sim_split (exact 3-way bf16 split, six piece products on the bf16 matrix cores) is
    held to what the fp32 kernel delivers, measured against float64: maxima within 1e-6 of the
    scale sum|a_k b_k| (+ norms) -- the bound is 2^-23 from the dropped products plus accumulation
    rounding -- and no worse than 4x the fp32 kernel's own worst error; the arg-max is the float64
    arg-max or a near-tie (gap <= 2e-6 of the scale); ragged shapes: d not a multiple of 16, n not a
    multiple of 32, n > 256 (second pass folds into the first), m below one block."""
    rng = np.random.default_rng(l * 1000 + d * 10 + n)
    A = (rng.standard_normal((l, d, m)) * scale).astype(np.float32)
    B = (A[:, :, rng.integers(0, m, n)] + 0.1 * scale * rng.standard_normal((l, d, n))).astype(np.float32)
    B[:, :, n // 2] = B[:, :, 0]  # duplicate centroid: exact tie -> smallest index
    assert K.MaxSimHip.split_supported(d, m, n)
    sims, mag = _max_sim_f64(A, B, distance)
    best = sims.max(axis=2)
    err = {}
    for prec in ("fp32", "bf16x3"):
        v, i = K.MaxSimHip(distance=distance, precision=prec)(T(A), T(B), dim=2, mode="tn")
        v, i = N(v), N(i)
        assert i.dtype == np.int64 and i.min() >= 0 and i.max() < n
        at = np.take_along_axis(sims, i[:, :, None], 2)[:, :, 0]
        sc = np.take_along_axis(mag, i[:, :, None], 2)[:, :, 0]
        err[prec] = (np.abs(v - at) / sc).max()
        assert err[prec] <= 1e-6, (prec, err[prec])
        assert ((best - at) <= 2e-6 * sc).all(), prec
        if prec == "bf16x3":  # the duplicate never beats its original
            assert not (i == n // 2).any()
            # against the bit-exact kernel: the same labels except at float64 near-ties
            ie = N(K.MaxSimHip(distance=distance)(T(A), T(B), dim=2, mode="tn")[1])
            ate = np.take_along_axis(sims, ie[:, :, None], 2)[:, :, 0]
            assert (i == ie).mean() >= 0.99
            assert (np.abs(at - ate)[i != ie] <= 4e-6 * sc[i != ie]).all(), \
                (np.argwhere(i != ie), (np.abs(at - ate) / sc)[i != ie])
    assert err["bf16x3"] <= 4 * err["fp32"] + 1e-8, err


def test_max_sim_split_is_exact_on_small_integers(K):
    """SIFT-like data (integers 0..255) and integer centroids: every value is one bf16 piece, all
    products and sums are exact in fp32, so the split kernel returns the oracle's bits"""
    rng = np.random.default_rng(5)
    A = rng.integers(0, 256, (2, 32, 2000)).astype(np.float32)
    B = rng.integers(0, 256, (2, 32, 256)).astype(np.float32)
    v, i = K.MaxSimHip(distance="euclidean", precision="bf16x3")(T(A), T(B), dim=2, mode="tn")
    ev, ei = c_oracle.max_sim(A, B, "euclidean", "expanded")
    assert np.array_equal(N(i), ei) and np.array_equal(N(v), ev)


def test_max_sim_split_rejects_what_it_does_not_cover(K):
    from torchpq_amd import _lib
    lib = _lib.load()
    assert not K.MaxSimHip.split_supported(65, 1000, 256)
    assert not K.MaxSimHip.split_supported(64, 2 ** 24, 256)  # padded slice >= 2 GiB
    A, B = T(np.zeros((1, 65, 8), np.float32)), T(np.zeros((1, 65, 4), np.float32))
    v, i = torch.empty(1, 8, device=DEV), torch.empty(1, 8, device=DEV, dtype=torch.int64)
    rc = lib.tpq_max_sim_split(_lib.ptr(A), _lib.ptr(B), _lib.ptr(v), _lib.ptr(i), 1, 65, 8, 4,
                               _lib.METRIC_NEG_SQ_L2, _lib.stream_ptr(DEV))
    assert rc == _lib.ERR_UNSUPPORTED and b"max_sim_split" in lib.tpq_last_error()
    # the wrapper falls back to the fp32 kernel for such shapes
    A = T(np.random.default_rng(0).standard_normal((1, 65, 100)).astype(np.float32))
    B = A[:, :, :7].contiguous()
    v1, i1 = K.MaxSimHip(precision="bf16x3")(A, B, dim=2)
    v0, i0 = K.MaxSimHip()(A, B, dim=2)
    assert torch.equal(v1, v0) and torch.equal(i1, i0)


def test_max_sim_and_centroids_match_reference_golden(K, fx_kmeans):
    fx = fx_kmeans
    v, lab = K.MaxSimHip()(T(fx["data"]), T(fx["init"]), dim=2, mode="tn")
    lab, v = N(lab), N(v)
    same = lab[:, :-1] == fx["ref_labels"]
    assert same.mean() > 0.999
    gap = fx["ref_sims_top2gap"][:, :-1]
    assert np.all(gap[~same] <= 1e-3 * np.abs(fx["ref_maxsims"][~same]) + 1e-3)
    np.testing.assert_allclose(v[:, :-1][same], fx["ref_maxsims"][same], rtol=1e-4, atol=1e-2)
    cen = N(K.ComputeCentroidsHip()(T(fx["data"]), T(fx["labels_for_update"]), k=fx["init"].shape[2]))
    np.testing.assert_allclose(cen, fx["ref_centroids"], rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("l,d,n,k", [(1, 5, 1000, 7), (3, 40, 9000, 256), (2, 17, 100, 1024),
                                     (1, 24, 30000, 16384)])
def test_compute_centroids(K, l, d, n, k):
    rng = np.random.default_rng(n + k)
    data = rng.standard_normal((l, d, n)).astype(np.float32)
    labels = rng.integers(0, max(1, k - 2), (l, n)).astype(np.int64)  # last clusters stay empty
    got = N(K.ComputeCentroidsHip()(T(data), T(labels), k=k))
    exp = orc.compute_centroids(data, labels, k)
    np.testing.assert_allclose(got, exp, rtol=1e-5, atol=1e-5)
    assert np.all(got[:, :, k - 1] == 0)  # empty cluster -> 0 (compute_centroids.cu:82)


# ---------------------------------------------------------------------------------------------
# container helpers
# ---------------------------------------------------------------------------------------------
def test_get_ioa(K):
    rng = np.random.default_rng(3)
    for n, n_cells in [(1, 4), (1000, 5), (50000, 1024), (4097, 16384)]:
        cells = rng.integers(0, n_cells, n).astype(np.int64)
        got = N(K.GetIOAHip()(T(cells), n_cells=n_cells))
        assert np.array_equal(got, orc.get_ioa(cells))


def test_get_write_address_and_cell_by_address(K):
    rng = np.random.default_rng(4)
    n_cells = 9
    cap = rng.integers(0, 200, n_cells).astype(np.int64)
    cap[2] = 0
    start = np.cumsum(cap) - cap
    total = int(cap.sum())
    is_empty = (rng.random(total) < 0.6).astype(np.uint8)
    cells = rng.integers(0, n_cells, 400).astype(np.int64)
    ioa = orc.get_ioa(cells)
    got = N(K.GetWriteAddressHip()(T(is_empty), T(start), T(cap), T(cells), T(ioa)))
    assert np.array_equal(got, orc.get_write_address(is_empty, start, cap, cells, ioa))
    adr = np.arange(-3, total + 3).astype(np.int64)
    got = N(K.GetCellByAddressHip()(T(adr), T(start), T(start + cap)))
    assert np.array_equal(got, orc.get_cell_by_address(adr, start, cap))


def test_pq_decode_and_scatter(K, fx_tiny):
    cb = _sd(fx_tiny, "pq_codec.kmeans.centroids")
    got = N(K.PQDecodeHip()(T(cb), T(fx_tiny["ref_decode_codes"])))
    assert np.array_equal(got, fx_tiny["ref_decode"])
    rng = np.random.default_rng(8)
    m, cap, n = 16, 500, 120
    storage = np.zeros((m // 4, cap, 4), np.uint8)
    codes = rng.integers(0, 256, (m, n), dtype=np.uint8)
    adr = rng.choice(cap, n, replace=False).astype(np.int64)
    adr[5] = -1
    adr[6] = cap + 4
    st = T(storage)
    pk = K.PackCodesHip()(st)
    K.ScatterCodesHip()(T(codes), T(adr), st, pk)
    orc.codes_to_storage(codes, adr, storage)
    assert np.array_equal(N(st), storage)
    assert np.array_equal(N(pk), N(K.PackCodesHip()(st)))  # incremental == rebuilt
    a2i = rng.integers(-1, 50, cap).astype(np.int64)
    probe = rng.integers(-5, cap + 5, (7, 9)).astype(np.int64)
    assert np.array_equal(N(K.GetIdByAddressHip()(T(a2i), T(probe))), orc.get_id_by_address(a2i, probe))


# ---------------------------------------------------------------------------------------------
# residual PQ scan
# ---------------------------------------------------------------------------------------------
def test_residual_scan_matches_golden(K, fx_residual):
    fx = fx_residual
    m = int(fx["m"])
    scan = K.IVFPQTopkHip(m=m)
    cells = fx["ref_cells"]
    st = T(_sd(fx, "_storage"))
    cs, sz = T(_sd(fx, "_cell_start")[cells]), T(_sd(fx, "_cell_size")[cells])
    nq, n_probe = cells.shape
    npl = T(np.full(nq, n_probe, np.int64))
    a2i = T(_sd(fx, "_address2id"))
    for k in (1, 10, 100):
        v, a, i = scan.topk_residual_precomputed(st, T(fx["ref_part1"]), T(fx["ref_part2"]), T(cells),
                                                 T(fx["ref_topk_sims"]), T(_sd(fx, "_is_empty")), cs, sz,
                                                 npl, n_candidates=k, address2id=a2i)
        assert np.array_equal(N(v), fx[f"orc_vals_k{k}"]) and np.array_equal(N(a), fx[f"orc_addr_k{k}"])
        assert np.array_equal(N(i), orc.get_id_by_address(_sd(fx, "_address2id"), fx[f"orc_addr_k{k}"]))
        v2, a2 = scan.topk_residual(st, T(fx["ref_full"]), T(fx["ref_topk_sims"]), None, cs, sz, npl,
                                    n_candidates=k)
        assert np.array_equal(N(v2), fx[f"orc_full_vals_k{k}"])
        assert np.array_equal(N(a2), fx[f"orc_full_addr_k{k}"])
    p1 = N(K.ResidualPart1Hip()(T(fx["queries"]), T(_sd(fx, "pq_codec.kmeans.centroids"))))
    assert np.array_equal(p1, orc.residual_part1(fx["queries"], _sd(fx, "pq_codec.kmeans.centroids")))
    np.testing.assert_allclose(p1, fx["ref_part1"], rtol=1e-4, atol=1e-5 * np.abs(fx["ref_part1"]).max())


@pytest.mark.parametrize("m,k,n_probe,tomb", [(8, 10, 5, 0), (64, 100, 12, 30), (16, 300, 7, 0), (24, 1, 9, 5)])
def test_residual_scan_random_vs_oracle(K, m, k, n_probe, tomb):
    rng = np.random.default_rng(m * 7 + k)
    n_cells, nq = 30, 21
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 140, tomb, 0.1)
    part1 = (rng.standard_normal((nq, m, 256)) * 50).astype(np.float32)
    part2 = (rng.standard_normal((n_cells, m, 256)) * 50).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    cells[2, 1] = cells[2, 0]
    base = (rng.standard_normal((nq, n_probe)) * 300).astype(np.float32)
    npl = rng.integers(0, n_probe + 1, nq).astype(np.int64)
    npl[:4] = n_probe
    cs, sz = start[cells], sizes[cells]
    ev, ea = c_oracle.scan_topk_residual(storage, part1, part2, cells, base, is_empty, cs, sz, npl, k)
    scan = K.IVFPQTopkHip(m=m)
    v, a = scan.topk_residual_precomputed(T(storage), T(part1), T(part2), T(cells), T(base),
                                          T(is_empty), T(cs), T(sz), T(npl), n_candidates=k)
    assert np.array_equal(N(v), ev) and np.array_equal(N(a), ea)


@pytest.mark.parametrize("m,k,n_probe,tomb,mode", [
    (8, 10, 5, 0, "part1"), (64, 100, 12, 30, "part1"), (16, 300, 7, 0, "fused"), (32, 1, 9, 5, "fused"),
    (120, 60, 6, 0, "part1"), (64, 100, 12, 0, "ties"), (16, 20, 8, 3, "dup"), (64, 1020, 9, 0, "part1")])
def test_residual_packed_scan_vs_oracle(K, m, k, n_probe, tomb, mode):
    """tpq_ivfpq_scan_topk_residual_packed == the residual oracle, bit for bit (values, addresses),
    incl. splits, tombstones, mass ties (band overflow -> exact redo) and a cell listed twice."""
    rng = np.random.default_rng(m * 11 + k)
    n_cells, nq = 30, 21
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 140, tomb, 0.1)
    part2 = (rng.standard_normal((n_cells, m, 256)) * 50).astype(np.float32)
    ds, query, cb = 2, None, None
    if mode == "fused":
        cb = (rng.standard_normal((m, ds, 256)) * 8).astype(np.float32)
        query = (rng.standard_normal((m * ds, nq)) * 8).astype(np.float32)
        part1 = orc.residual_part1(query, cb)
    elif mode == "ties":  # small integers: thousands of exactly equal values
        part1 = rng.integers(-1, 2, (nq, m, 256)).astype(np.float32)
        part2 = rng.integers(-1, 2, (n_cells, m, 256)).astype(np.float32)
    else:
        part1 = (rng.standard_normal((nq, m, 256)) * 50).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    cells[2, 1] = cells[2, 0]          # adjacent repeat: skipped (ivfpq_topk.cu:1092-1107)
    if mode == "dup":
        cells[3, 4] = cells[3, 1]      # non-adjacent repeat: the cell is scanned twice
        cells[5, 7] = cells[5, 0]
    base = (rng.standard_normal((nq, n_probe)) * 300).astype(np.float32)
    if mode == "ties":
        base = np.round(base / 100).astype(np.float32)
    npl = rng.integers(0, n_probe + 1, nq).astype(np.int64)
    npl[:8] = n_probe
    cs, sz = start[cells], sizes[cells]
    ev, ea = c_oracle.scan_topk_residual(storage, part1, part2, cells, base, is_empty, cs, sz, npl, k)
    scan = K.IVFPQTopkHip(m=m)
    st, p2 = T(storage), T(part2)
    packed = K.PackCodesHip()(st)
    slot_term, cell_bound = K.ResidualSlotTermsHip()(st, p2, T(start), T(sizes))
    # the per-slot constant is the ascending-j fp32 sum of the slot's part2 entries
    stn, codes = N(slot_term), orc.storage_to_codes(storage, np.arange(storage.shape[1]))
    for s in rng.integers(0, storage.shape[1], 50):
        c = np.searchsorted(start, s, side="right") - 1
        if s < start[c] + sizes[c]:
            acc = np.float32(0)
            for j in range(m):
                acc = np.float32(acc + part2[c, j, codes[j, s]])
            assert stn[s] == acc
    np.testing.assert_allclose(N(cell_bound), np.abs(part2).max(-1).sum(-1), rtol=1e-5)
    for n_split in (1, 3):
        v, a = scan.topk_residual_packed(
            st, packed, p2, slot_term, cell_bound, T(cells), T(base), T(is_empty), T(cs), T(sz), T(npl),
            n_candidates=k, part1=None if mode == "fused" else T(part1),
            query=T(query) if mode == "fused" else None, codebook=T(cb) if mode == "fused" else None,
            n_split=n_split)
        assert np.array_equal(N(v), ev) and np.array_equal(N(a), ea), (mode, n_split)


@pytest.mark.parametrize("m,ds,k,layout,distance", [(64, 2, 100, "packed", "euclidean"), (16, 4, 10, "packed", "cosine"),
                                                    (120, 8, 50, "packed", "euclidean"), (24, 3, 7, "ref", "euclidean"),
                                                    (8, 16, 130, "ref", "euclidean")])
def test_fused_lut_scan_equals_lut_then_scan(K, m, ds, k, layout, distance):
    """tpq_ivfpq_search_fused (LUT built inside the scan workgroups) == tpq_adc_lut + scan, bit for bit."""
    rng = np.random.default_rng(m + ds + k)
    n_cells, nq, n_probe = 30, 33, 9
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 160, 0, 0.0)
    cb = (rng.standard_normal((m, ds, 256)) * 20).astype(np.float32)
    q = (rng.standard_normal((m * ds, nq)) * 20).astype(np.float32)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    npl = rng.integers(1, n_probe + 1, nq).astype(np.int64)
    cs, sz = T(start[cells]), T(sizes[cells])
    scan = K.IVFPQTopkHip(m=m)
    st = T(storage)
    packed = K.PackCodesHip()(st) if layout == "packed" else None
    lut = K.AdcLutHip()(T(q), T(cb), distance)
    for n_split in (1, 2):
        v0, a0 = scan.topk(st, lut, None, cs, sz, T(npl), n_candidates=k, packed=packed, n_split=n_split)
        v1, a1, i1 = scan.topk_fused(st, T(q), T(cb), None, cs, sz, T(npl), n_candidates=k,
                                     distance=distance, packed=packed, address2id=T(a2i), n_split=n_split)
        assert torch.equal(v0, v1) and torch.equal(a0, a1)
    ev, ea = c_oracle.scan_topk(storage, c_oracle.adc_lut(q, cb, distance), is_empty, start[cells],
                                sizes[cells], npl, k)
    assert np.array_equal(N(v1), ev) and np.array_equal(N(a1), ea)


def test_coarse_select_equals_metric_then_select(K):
    """tpq_coarse_select == metric.negative_squared_l2_distance + tpq_topk_select, bit for bit."""
    from torchpq_amd import metric
    g = torch.Generator(device=DEV)
    g.manual_seed(3)
    x = torch.randn(128, 777, generator=g, device=DEV) * 30
    c = torch.randn(128, 1024, generator=g, device=DEV) * 30
    sims = metric.negative_squared_l2_distance(x, c).contiguous()
    for k in (1, 32, 64):
        v0, i0 = K.TopkSelectHip()(sims, k=k)
        dots = x.transpose(0, 1).contiguous() @ c
        v1, i1 = K.CoarseSelectHip()(dots, (x * x).sum(0), (c * c).sum(0), k)
        assert torch.equal(v0, v1) and torch.equal(i0, i1)
        ev, ei = orc.topk_desc(N(sims), k)
        assert np.array_equal(N(v1), ev) and np.array_equal(N(i1), ei)


@pytest.mark.parametrize("d,nq,n_cells,n_probe,smart", [(128, 777, 1024, 32, True), (32, 5, 16, 16, False),
                                                       (960, 70, 300, 64, True), (7, 1, 40, 1, True),
                                                       (128, 130, 2000, 200, True),
                                                       # big enough for the 128-centroid x 256-query GEMM blocks
                                                       (32, 1100, 16500, 8, True), (24, 1300, 8200, 64, False),
                                                       (16, 2100, 4100, 300, True)])
def test_coarse_probe_fused(K, d, nq, n_cells, n_probe, smart):
    """tpq_ivfpq_coarse_probe: sims within fp32 tolerance of the oracle's (float64-accumulated)
    metric, the selection EXACT on the kernel's own sims, extents gathered, probe counts equal to
    tpq_smart_probing on the same sims."""
    rng = np.random.default_rng(d + nq)
    x = (rng.standard_normal((d, nq)) * 20).astype(np.float32)
    c = (rng.standard_normal((d, n_cells)) * 20).astype(np.float32)
    sizes = rng.integers(0, 500, n_cells).astype(np.int64)
    start = (np.cumsum(sizes + 3) - sizes - 3).astype(np.int64)
    sims, cells, cs, sz, npl = K.CoarseProbeHip()(T(x), T(c), T(start), T(sizes), n_probe,
                                                  30.0 if smart else None)
    sims, cells = N(sims), N(cells)
    exact = -((x.astype(np.float64).T[:, None, :] - c.astype(np.float64).T[None]) ** 2).sum(-1)
    scale = np.abs(exact).max()
    got_at = np.take_along_axis(exact, cells, axis=1)
    np.testing.assert_allclose(sims, got_at, rtol=1e-4, atol=1e-6 * scale)
    assert (np.diff(sims, axis=1) <= 0).all()
    # the chosen set is the top-n_probe up to fp32 noise at the boundary
    kth = -np.sort(-exact, axis=1)[:, n_probe - 1]
    assert (got_at >= kth[:, None] - 2e-4 * scale).all()
    assert all(len(set(r)) == n_probe for r in cells)
    assert np.array_equal(N(cs), start[cells]) and np.array_equal(N(sz), sizes[cells])
    if smart and n_probe > 1:
        assert np.array_equal(N(npl), N(K.SmartProbingHip()(T(sims), 30.0)))
    else:
        assert np.array_equal(N(npl), np.full(nq, n_probe))


@pytest.mark.parametrize("name", ["fx_c1", "fx_ties", "fx_tomb"])
@pytest.mark.parametrize("layout", ["ref", "packed"])
def test_scan_on_reference_built_fixtures(K, name, layout, request):
    """C1-shaped index, reference-made duplicates (exact ties) and tombstones inside cells: values,
    addresses and ids equal the committed vectors for both code layouts and any split."""
    fx = request.getfixturevalue(name)
    m = int(fx["m"])
    scan = K.IVFPQTopkHip(m=m)
    storage = T(_sd(fx, "_storage"))
    packed = K.PackCodesHip()(storage) if layout == "packed" else None
    a2i = T(_sd(fx, "_address2id"))
    cs = T(_sd(fx, "_cell_start")[fx["ref_cells"]])
    sz = T(_sd(fx, "_cell_size")[fx["ref_cells"]])
    nq = int(fx["nq"])
    npl = T(np.full(nq, int(fx["n_probe"]), np.int64))
    for k in fx["ks"]:
        k = int(k)
        key = "s0_k%d" % k if name == "fx_c1" else "k%d" % k
        for n_split in (1, 4):
            v, a, i = scan.topk(storage, T(fx["ref_lut"]), T(_sd(fx, "_is_empty")), cs, sz, npl,
                                n_candidates=k, packed=packed, address2id=a2i, n_split=n_split)
            assert np.array_equal(N(v), fx["orc_vals_" + key])
            assert np.array_equal(N(a), fx["orc_addr_" + key])
            assert np.array_equal(N(i), fx["orc_ids_" + key])


def test_code_layout_scatter_gather_matches_reference(K, fx_layout):
    """tpq_scatter_codes / get_data_by_address against the reference's own set/get (fx_layout)."""
    from torchpq_amd.container import CellContainer
    fx = fx_layout
    for case in range(3):
        m = int(fx[f"l{case}_m"])
        ref_storage = fx[f"l{case}_ref_storage"]
        cap = ref_storage.shape[1]
        st = torch.zeros(m // 4, cap, 4, dtype=torch.uint8, device=DEV)
        pk = K.PackCodesHip()(st)
        K.ScatterCodesHip()(T(fx[f"l{case}_codes"]), T(fx[f"l{case}_adr"]), st, pk)
        assert np.array_equal(N(st), ref_storage)
        assert np.array_equal(N(pk), N(K.PackCodesHip()(T(ref_storage))))
        n_cells = {0: 5, 1: 3, 2: 2}[case]
        c = CellContainer(code_size=m, n_cells=n_cells, device=DEV, initial_size=16,
                          expand_step_size=8, expand_mode="double", contiguous_size=4)
        assert c.capacity == cap
        c.set_data_by_address(T(fx[f"l{case}_codes"]), T(fx[f"l{case}_adr"]))
        assert np.array_equal(N(c._storage), ref_storage)
        assert np.array_equal(N(c.get_data_by_address(T(fx[f"l{case}_probe"]))), fx[f"l{case}_ref_gather"])


# ---------------------------------------------------------------------------------------------
# coarse assign: error-bounded selection on the bf16 matrix cores + exact re-check
# ---------------------------------------------------------------------------------------------
def _coarse_case(rng, d, m, n, kind):
    if kind == "gauss":
        A = (rng.standard_normal((d, m)) * 10).astype(np.float32)
        B = (rng.standard_normal((d, n)) * 10).astype(np.float32)
    elif kind == "sift":  # non-negative integers, centroids near data points
        A = rng.integers(0, 200, (d, m)).astype(np.float32)
        B = (A[:, rng.integers(0, m, n)] + rng.integers(-3, 4, (d, n))).astype(np.float32)
    elif kind == "crowded":  # every centroid within a few ulps of the same vector: all points ambiguous
        A = (rng.standard_normal((d, m)) * 10).astype(np.float32)
        c0 = (rng.standard_normal((d, 1)) * 10).astype(np.float32)
        B = np.nextafter(np.repeat(c0, n, 1), np.float32(np.inf) * rng.choice([-1, 1], (d, n))).astype(np.float32)
        B[:, ::3] = c0  # and exact duplicates: ties -> smallest index
    else:  # "ties": duplicated centroids, points sitting on centroids
        B = (rng.standard_normal((d, n)) * 5).astype(np.float32)
        B[:, n // 2:] = B[:, :n - n // 2]
        A = B[:, rng.integers(0, n, m)].copy()
        A[:, ::2] += (rng.standard_normal((d, (m + 1) // 2)) * 0.01).astype(np.float32)
    return np.ascontiguousarray(A), np.ascontiguousarray(B)


@pytest.mark.parametrize("d,m,n,kind", [(128, 3000, 1024, "sift"), (128, 1111, 300, "gauss"),
                                        (100, 2000, 129, "gauss"), (17, 5000, 64, "sift"),
                                        (64, 700, 2049, "ties"), (128, 600, 500, "crowded"),
                                        (64, 40000, 300, "crowded"),  # more re-checked points than the compact copy holds
                                        (33, 513, 31, "ties"), (96, 40, 4000, "gauss"),
                                        (1, 300, 5, "gauss")])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_coarse_assign_labels_equal_the_exact_kernel_and_the_oracle(K, d, m, n, kind, distance):
    """tpq_coarse_assign decides on a split-bf16 top-2 with a rigorous error bound and re-checks the
    ambiguous points with the fp32 kernel: its labels are the oracle's, bit for bit -- on ragged
    shapes (d not a multiple of 16, n not a multiple of 128, m below a block), exact ties
    (duplicated centroids -> smallest index), points sitting on centroids, and a codebook whose
    entries differ by single ulps (every point ambiguous: the answer comes from the re-check)."""
    rng = np.random.default_rng(d * 1000 + n)
    A, B = _coarse_case(rng, d, m, n, kind)
    assert K.CoarseAssignHip.supported(d, m, n)
    op = K.CoarseAssignHip(distance=distance)
    got = N(op(T(A), T(B)))
    _, want = c_oracle.max_sim(A[None], B[None], distance, "expanded")
    assert got.dtype == np.int64 and np.array_equal(got, want[0])
    share = op.last_rechecked() / m
    if kind == "crowded":
        assert share == 1.0   # nothing can be decided by the fast values
    elif kind == "gauss" and d >= 64 and distance == "euclidean":
        assert share < 0.5    # ... and normally most points are


def test_coarse_assign_argument_errors(K):
    from torchpq_amd import _lib
    lib = _lib.load()
    assert K.CoarseAssignHip.supported(129, 1000, 256)      # (wide vectors: tests/test_gpu_wide_assign.py)
    assert not K.CoarseAssignHip.supported(1025, 1000, 256)
    A, B = T(np.zeros((1025, 8), np.float32)), T(np.zeros((1025, 4), np.float32))
    out = torch.empty(8, device=DEV, dtype=torch.int64)
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    rc = lib.tpq_coarse_assign(_lib.ptr(A), _lib.ptr(B), None, _lib.ptr(out), 1025, 8, 4, _lib.METRIC_NEG_SQ_L2,
                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    assert rc == _lib.ERR_UNSUPPORTED and b"coarse_assign" in lib.tpq_last_error()
    A, B = T(np.zeros((64, 800), np.float32)), T(np.zeros((64, 400), np.float32))
    need = lib.tpq_coarse_assign_workspace_bytes(64, 800, 400)
    assert need > 0
    out = torch.empty(800, device=DEV, dtype=torch.int64)
    rc = lib.tpq_coarse_assign(_lib.ptr(A), _lib.ptr(B), None, _lib.ptr(out), 64, 800, 400, _lib.METRIC_NEG_SQ_L2,
                               _lib.ptr(ws), need - 1, _lib.stream_ptr(DEV))
    assert rc == -1 and b"workspace" in lib.tpq_last_error()
    # all-zero data: every centroid ties -> index 0
    rc = lib.tpq_coarse_assign(_lib.ptr(A), _lib.ptr(B), None, _lib.ptr(out), 64, 800, 400, _lib.METRIC_NEG_SQ_L2,
                               _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    assert rc == 0 and int(out.abs().max()) == 0


@pytest.mark.parametrize("l,d,m,n,kind", [(3, 64, 3000, 256, "gauss"), (2, 40, 2500, 200, "sift"),
                                          (1, 17, 5000, 37, "gauss"), (2, 64, 700, 256, "ties"),
                                          (2, 32, 600, 250, "crowded"), (4, 12, 300, 5, "gauss"),
                                          (1, 48, 40, 256, "sift")])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_max_sim_select_labels_equal_the_oracle(K, l, d, m, n, kind, distance):
    """tpq_max_sim_select (batched, centroids resident): the bounded bf16 top-2 selection + exact
    re-check gives the oracle's labels, bit for bit, for every sub-problem -- ragged shapes, exact
    ties, points on centroids, single-ulp codebooks; the maxima it returns are within 2e-4."""
    rng = np.random.default_rng(l * 100 + d * 7 + n)
    As, Bs = zip(*[_coarse_case(rng, d, m, n, kind) for _ in range(l)])
    A, B = np.stack(As), np.stack(Bs)
    assert K.MaxSimSelectHip.supported(l, d, m, n)
    v, i = K.MaxSimSelectHip(distance=distance)(T(A), T(B))
    ev, ei = c_oracle.max_sim(A, B, distance, "expanded")
    assert N(i).dtype == np.int64 and np.array_equal(N(i), ei)
    scale = np.abs(ev).max() + 1e-6
    assert np.abs(N(v) - ev).max() <= 2e-4 * max(scale, float((A * A).sum(1).max()))


def test_max_sim_select_argument_errors(K):
    from torchpq_amd import _lib
    lib = _lib.load()
    assert not K.MaxSimSelectHip.supported(2, 65, 100, 256)
    assert not K.MaxSimSelectHip.supported(2, 64, 100, 257)
    A, B = T(np.zeros((2, 64, 8), np.float32)), T(np.zeros((2, 64, 300), np.float32))
    v = torch.empty(2, 8, device=DEV)
    i = torch.empty(2, 8, device=DEV, dtype=torch.int64)
    ws = torch.empty(1 << 20, device=DEV, dtype=torch.uint8)
    rc = lib.tpq_max_sim_select(_lib.ptr(A), _lib.ptr(B), _lib.ptr(v), _lib.ptr(i), 2, 64, 8, 300,
                                _lib.METRIC_NEG_SQ_L2, _lib.ptr(ws), ws.numel(), _lib.stream_ptr(DEV))
    assert rc == _lib.ERR_UNSUPPORTED and b"max_sim_select" in lib.tpq_last_error()


def test_selection_kernels_degenerate_shapes(K):
    """one point, one centroid, no point: tpq_coarse_assign / tpq_max_sim_select behave like the exact kernel"""
    rng = np.random.default_rng(0)
    for d, m, n in ((128, 1, 1), (5, 1, 300), (64, 513, 1), (16, 0, 7)):
        A = rng.standard_normal((d, m)).astype(np.float32)
        B = rng.standard_normal((d, n)).astype(np.float32)
        got = N(K.CoarseAssignHip()(T(A), T(B)))
        assert got.shape == (m,)
        if m:
            _, want = c_oracle.max_sim(A[None], B[None], "euclidean", "expanded")
            assert np.array_equal(got, want[0])
    for l, d, m, n in ((1, 64, 1, 1), (3, 20, 1, 256), (2, 48, 300, 1), (2, 32, 0, 9)):
        A = rng.standard_normal((l, d, m)).astype(np.float32)
        B = rng.standard_normal((l, d, n)).astype(np.float32)
        v, i = K.MaxSimSelectHip()(T(A), T(B))
        assert tuple(i.shape) == (l, m) and tuple(v.shape) == (l, m)
        if m:
            _, want = c_oracle.max_sim(A, B, "euclidean", "expanded")
            assert np.array_equal(N(i), want)


def test_selection_kernels_random_soak():
    """tools/selection_soak.py, 24 random cases: shapes and data kinds at random (Gaussian, SIFT-like,
    heavy-tailed, tight clusters, large common offset, tiny / huge magnitudes, duplicated centroids);
    both selection kernels must return the fp32 kernel's labels on every one (1 600 cases of the same
    tool were run once by hand: none differed)"""
    import subprocess
    import sys as _sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([_sys.executable, os.path.join(root, "tools", "selection_soak.py"), "--cases", "24",
                        "--seed", "7"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
