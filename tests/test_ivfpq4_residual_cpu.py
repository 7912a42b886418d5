"""CPU: the residual codes of IVFPQ4Index -- the oracle's per-probe tables and values (tests/ivfpq4_residual_oracle.py
restates include/torchpq_amd.h) against float64 and against the plain oracle, its order, candidates and padding, the
premise of the GPU summation-order case, and the argument checks of tpq_ivfpq4_scan_residual_topk and of the Python
layers, which run before any HIP call."""
import ctypes

import numpy as np
import pytest

import ivfpq4_cases as plain_cases
import ivfpq4_oracle as porc
import ivfpq4_residual_cases as cases
import ivfpq4_residual_oracle as rorc


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
@pytest.mark.parametrize("m,ds", [(8, 5), (64, 2), (256, 1)])
def test_oracle_tables_and_values_against_float64(m, ds, distance):
    """Against metric(q, centroid + codeword) in float64.  Every fp32 operation rounds by at most u = 2^-24 relative.
    The reconstruction y = centroid + codeword is one rounded add: |y - y64| <= u (|centroid| + |codeword|) =: u Y.
    Euclidean, one step: t = q - y carries that error and its own rounding, |t - t64| <= u Y + u |t64| to first order,
    so t*t is within 2 |t64| u (Y + |t64|) + u t64^2 of t64^2; with A := t64^2 + 2 |t64| Y that is <= 3 u A, and the
    running sum (each partial sum <= the sum of the A) adds u per step: an entry is within (3 + ds) u sum(A).
    Inner: q*y is within u |q| Y + u |q y64| <= 2 u |q| Y =: 2 u A; an entry within (2 + ds) u sum(A).
    2 x 3 ds u sum(A) is used for both, as tests/test_ivfpq4_cpu.py does for the plain table.
    A value adds m entries, every partial sum no larger than S = the sum of the entries' sum(A): within
    (3 + ds + m) u S to first order, and 2 (3 ds + m) u S is used."""
    rng = np.random.default_rng(100 + m + ds)
    nq, n_probe, n_cells, cap = 5, 3, 6, 40
    cb = rng.standard_normal((m, ds, 16)).astype(np.float32)
    cen = rng.standard_normal((n_cells, m * ds)).astype(np.float32)
    query = rng.standard_normal((m * ds, nq)).astype(np.float32)
    cells = rng.integers(0, n_cells, (nq, n_probe)).astype(np.int64)
    codes = rng.integers(0, 16, (m, cap)).astype(np.uint8)
    table = rorc.lut(query, cb, cen, cells, distance)
    assert table.shape == (nq, n_probe, m, 16) and table.dtype == np.float32
    q64 = query.astype(np.float64).T.reshape(nq, 1, m, ds, 1)
    c64 = cen.astype(np.float64)[cells].reshape(nq, n_probe, m, ds, 1)
    w64 = cb.astype(np.float64)[None, None]                                  # [1, 1, m, ds, 16]
    y64 = c64 + w64
    big_y = np.abs(c64) + np.abs(w64)
    if distance == "euclidean":
        t64 = q64 - y64
        terms, mag = -t64 ** 2, t64 ** 2 + 2 * np.abs(t64) * big_y
    else:
        terms, mag = q64 * y64, np.abs(q64) * big_y
    e64, mag = terms.sum(3), mag.sum(3)                                      # [nq, n_probe, m, 16]
    assert np.all(np.abs(table - e64) <= 2 * 3 * ds * 2.0 ** -24 * mag)
    # every slot under every (query, probe)
    qi, pi, si = [x.ravel() for x in np.meshgrid(np.arange(nq), np.arange(n_probe), np.arange(cap), indexing="ij")]
    v = rorc.values(table, codes, qi, pi, si)
    assert v.shape == (nq * n_probe * cap,) and v.dtype == np.float32
    j = np.arange(m)[:, None]
    v64 = e64[qi[None, :], pi[None, :], j, codes[:, si]].sum(0)
    s64 = mag[qi[None, :], pi[None, :], j, codes[:, si]].sum(0)
    assert np.all(np.abs(v - v64) <= 2 * (3 * ds + m) * 2.0 ** -24 * s64)
    assert np.abs(v - v64).max() > 0          # (float32 was used: the comparison is not vacuous)


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
@pytest.mark.parametrize("m,ds,nq,n_probe,k", [(8, 5, 3, 4, 10), (24, 2, 70, 8, 100), (64, 1, 3, 8, 1024)])
def test_zero_centroids_give_the_plain_oracle_bit_for_bit(m, ds, nq, n_probe, k, distance):
    c = cases.case(7 * m + ds, m, ds, nq, n_probe)
    c["centroids"][:] = 0.0
    v, a = cases.scan(c, k, distance)
    pv, pa = porc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"], c["cs"], c["sz"], c["npl"], k,
                            distance)
    assert np.array_equal(a, pa) and np.array_equal(v.view(np.uint32), pv.view(np.uint32))
    assert (a >= 0).any()
    # ... and other centroids give other values
    c["centroids"][:] = 1.0
    v1, _ = cases.scan(c, k, distance)
    assert not np.array_equal(v1.view(np.uint32), pv.view(np.uint32))


def test_case_builder_keeps_the_plain_case_and_adds_cells_and_centroids():
    c = cases.case(31, 16, 2, 5, 4)
    p = plain_cases.case(31, 16, 2, 5, 4)
    for key in p:
        assert np.array_equal(c[key], p[key]), key
    assert c["cells"].shape == (5, 4) and c["cells"].dtype == np.int64
    assert c["centroids"].shape == (len(cases.CELL_SIZES), 32) and c["centroids"].dtype == np.float32
    assert c["cells"][1, 1] == c["cells"][1, 0]                       # the duplicated probe


def _tiny(codes, n_cells):
    """m = 8, ds = 1 storage from codes [8, cap]; codebook[j][0][c] = c for j == 0, else 0; centroid of cell i is
    (100 i, 0, ...): with an all-ones query and the inner product a slot's value is 100 cell + codes[0]"""
    cap = codes.shape[1]
    rows = porc.pack(codes)
    storage = np.ascontiguousarray(rows.reshape(1, 4, cap).transpose(0, 2, 1))
    cb = np.zeros((8, 1, 16), np.float32)
    cb[0, 0] = np.arange(16)
    cen = np.zeros((n_cells, 8), np.float32)
    cen[:, 0] = 100.0 * np.arange(n_cells)
    return storage, cb, cen


def test_oracle_order_on_ties_padding_and_duplicate_probe():
    codes = np.zeros((8, 12), np.uint8)
    codes[0] = [3, 7, 3, 7, 1, 7, 3, 0, 9, 9, 9, 9]
    storage, cb, cen = _tiny(codes, 3)
    query = np.ones((8, 1), np.float32)
    cs, sz = np.array([[0, 4]], np.int64), np.array([[4, 4]], np.int64)
    both = np.array([[1, 1]], np.int64)                        # both probes under centroid 1: the plain order + 100
    v, a = rorc.scan_topk(storage, query, cb, cen, both, None, cs, sz, np.array([2]), 6, "inner")
    assert a.tolist() == [[1, 3, 5, 0, 2, 6]] and v.tolist() == [[107, 107, 107, 103, 103, 103]]
    # the probe decides: slots 4 ... 7 under centroid 2, slots 0 ... 3 under centroid 0
    v, a = rorc.scan_topk(storage, query, cb, cen, np.array([[0, 2]], np.int64), None, cs, sz, np.array([2]), 6,
                          "inner")
    assert a.tolist() == [[5, 6, 4, 7, 1, 3]] and v.tolist() == [[207, 203, 201, 200, 7, 7]]
    # padding beyond the candidates
    v, a = rorc.scan_topk(storage, query, cb, cen, both, None, cs, sz, np.array([1]), 6, "inner")
    assert a.tolist() == [[1, 3, 0, 2, -1, -1]] and np.all(np.isneginf(v[0, 4:]))
    # tombstones
    empty = np.zeros(12, np.uint8)
    empty[[1, 5]] = 1
    v, a = rorc.scan_topk(storage, query, cb, cen, both, empty, cs, sz, np.array([2]), 3, "inner")
    assert a.tolist() == [[3, 0, 2]]
    # a probe whose start equals the previous probe's start is skipped, whatever its size and its cell: slots 0, 1
    # are valued under probe 0 (centroid 0) only; n_probe_list is clamped
    cs2, sz2 = np.array([[0, 0, 8]], np.int64), np.array([[2, 8, 4]], np.int64)
    cells2 = np.array([[0, 2, 1]], np.int64)
    v, a = rorc.scan_topk(storage, query, cb, cen, cells2, None, cs2, sz2, np.array([99]), 8, "inner")
    assert a.tolist() == [[8, 9, 10, 11, 1, 0, -1, -1]] and v[0, :6].tolist() == [109, 109, 109, 109, 7, 3]
    v, a = rorc.scan_topk(storage, query, cb, cen, cells2, None, cs2, sz2, np.array([-3]), 2, "inner")
    assert a.tolist() == [[-1, -1]]
    # a cell that leaves the storage is cut
    v, a = rorc.scan_topk(storage, query, cb, cen, np.array([[1]], np.int64), None, np.array([[10]], np.int64),
                          np.array([[50]], np.int64), np.array([1]), 4, "inner")
    assert a.tolist() == [[10, 11, -1, -1]]


def test_oracle_leaves_nan_values_out():
    codes = np.zeros((8, 6), np.uint8)
    codes[0] = [1, 2, 3, 4, 5, 6]
    storage, cb, cen = _tiny(codes, 2)
    cb[0, 0, 3] = np.nan
    cb[0, 0, 5] = -np.inf
    query = np.ones((8, 1), np.float32)
    v, a = rorc.scan_topk(storage, query, cb, cen, np.array([[1]], np.int64), None, np.array([[0]], np.int64),
                          np.array([[6]], np.int64), np.array([1]), 6, "inner")
    assert a.tolist() == [[5, 3, 1, 0, 4, -1]]       # -inf keeps its address, NaN never enters
    assert np.isneginf(v[0, 4]) and np.isneginf(v[0, 5]) and not np.isnan(v).any()
    # a NaN centroid takes its probe's slots out and leaves the other probe's
    cen[0, 3] = np.nan
    v, a = rorc.scan_topk(storage, query, cb, cen, np.array([[0, 1]], np.int64), None, np.array([[0, 3]], np.int64),
                          np.array([[3, 3]], np.int64), np.array([2]), 6, "inner")
    assert a.tolist() == [[5, 3, 4, -1, -1, -1]]


def test_summation_order_decides_places_in_the_offset_case():
    """the premise of test_gpu_ivfpq4_residual.test_scan_when_the_summation_order_decides: on those very inputs (seed
    4242, the plain offset case's, with every centroid component -2^20) an entry is centroid + codebook exactly, the
    partial sums reach -2^27, and a pairwise fp32 sum picks another top-k set than the specification's chain for at
    least one query (seen: it does, with the seed as it stands)"""
    c, k = cases.offset_case()
    assert cases.OFFSET_SEED == 4242
    p, _ = plain_cases.offset_case()
    assert np.array_equal(c["storage"], p["storage"]) and np.array_equal(c["codebook"], p["codebook"])
    table = rorc.lut(c["query"], c["codebook"], c["centroids"], c["cells"], "inner")
    want = (c["codebook"][:, 0, :] + np.float32(-2.0 ** 20)).astype(np.float32)
    assert np.array_equal(table, np.broadcast_to(want, table.shape))          # entries = centroid + codebook, exactly
    assert np.all(np.abs(table + 2.0 ** 21) < 8)
    ev, ea = cases.scan(c, k, "inner")
    assert ev[ea >= 0].min() < -2.0 ** 27 + 2.0 ** 12                         # the sums reach -2^27
    pairwise = cases.pairwise_topk_sets(c, k, "inner")
    differ = [q for q in range(len(pairwise)) if pairwise[q] != set(ea[q][ea[q] >= 0].tolist())]
    assert differ, "the two summation orders agree on every query: the case shows nothing"


def test_c_entry_point_checks_its_arguments_before_any_launch():
    from torchpq_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "tpq_ivfpq4_scan_residual_topk")
    assert lib.tpq_version() == 500

    def scan(m=16, ds=2, nq=4, max_nprobe=2, k=10, metric=0, n_split=1, n_slots=100, n_cells=8):
        return lib.tpq_ivfpq4_scan_residual_topk(None, None, None, None, None, n_cells, None, None, None, None, None,
                                                 None, n_slots, m, ds, nq, max_nprobe, k, metric, n_split, None, 0,
                                                 None)
    for bad_m in (0, 4, 12, 20, 257, 264, -8):
        assert scan(m=bad_m) == _lib.ERR_UNSUPPORTED and "m must be" in _lib.last_error(), bad_m
    assert scan(ds=0) == _lib.ERR_UNSUPPORTED
    for bad_k in (0, -1, 1025):
        assert scan(k=bad_k) == _lib.ERR_UNSUPPORTED and "k=" in _lib.last_error()
    assert scan(n_slots=2 ** 31 - 1) == _lib.ERR_UNSUPPORTED
    assert scan(metric=2) == -1 and scan(n_split=0) == -1 and scan(max_nprobe=0) == -1
    for bad_cells in (0, -5):
        assert scan(n_cells=bad_cells) == -1 and "n_cells" in _lib.last_error()
        assert scan(n_cells=bad_cells, nq=0) == -1
    assert scan() == -1 and "null pointer" in _lib.last_error()        # a supported shape gets as far as the pointers
    assert "ivfpq4_scan_residual" in _lib.last_error()
    assert scan(nq=0) == 0
    # every other pointer given (host memory: nothing reads it, the call returns before any launch): null centroids,
    # null cells, and a split call without its workspace
    buf = ctypes.create_string_buffer(64)
    some = ctypes.cast(buf, ctypes.c_void_p)

    def scan_with(centroids, cells, n_split=4):
        return lib.tpq_ivfpq4_scan_residual_topk(some, some, some, centroids, cells, 8, None, some, some, some, some,
                                                 some, 100, 16, 2, 4, 2, 10, 0, n_split, None, 0, None)
    assert scan_with(None, some) == -1 and "null pointer" in _lib.last_error()
    assert scan_with(some, None) == -1 and "null pointer" in _lib.last_error()
    assert scan_with(some, some) == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    short = lib.tpq_ivfpq4_scan_workspace_bytes(4, 10, 4) - 1
    assert lib.tpq_ivfpq4_scan_residual_topk(some, some, some, some, some, 8, None, some, some, some, some, some, 100,
                                             16, 2, 4, 2, 10, 0, 4, some, short, None) == _lib.ERR_WORKSPACE
    # the table buffers, the query and the probe table have to fit the LDS: declined, not launched
    assert lib.tpq_ivfpq4_scan_residual_topk(some, some, some, some, some, 8, None, some, some, some, some, some, 100,
                                             256, 160, 4, 2, 10, 0, 1, None, 0, None) == _lib.ERR_UNSUPPORTED
    assert "LDS" in _lib.last_error()


def test_python_layers_decline_unsupported_shapes():
    import torch
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFPQ4ResidualTopkHip
    for bad_m in (4, 12, 264):
        with pytest.raises(AssertionError):
            IVFPQ4ResidualTopkHip(m=bad_m)
    with pytest.raises(RuntimeError):
        from torchpq_amd.index import IVFPQ4Index
        IVFPQ4Index(32, 8, 16, device="cpu", pq_use_residual=True)
    c = cases.case(1, 8, 2, 2, 2)
    t = {key: torch.from_numpy(np.ascontiguousarray(val)) for key, val in c.items()}
    op = IVFPQ4ResidualTopkHip(m=8)

    def run(k=5, **other):
        a = dict(t, **other)
        return op(a["storage"], a["query"], a["codebook"], a["centroids"], a["cells"], a["cs"], a["sz"], a["npl"], k)
    for bad_k in (0, 1025):
        with pytest.raises(AssertionError):
            run(k=bad_k)
    with pytest.raises(AssertionError):
        run(centroids=t["centroids"][:, :-1])                    # another d than the codebook's
    with pytest.raises(AssertionError):
        run(centroids=t["centroids"][:0])                        # no cell
    with pytest.raises(AssertionError):
        run(cells=t["cells"][:, :1])                             # not the shape of cell_start
    with pytest.raises(AssertionError):
        run(cells=t["cells"].to(torch.int32))
    with pytest.raises(AssertionError):
        IVFPQ4ResidualTopkHip(m=16)(t["storage"], t["query"], t["codebook"], t["centroids"], t["cells"], t["cs"],
                                    t["sz"], t["npl"], 5)        # another m than the codebook's
    with pytest.raises(TorchPQAmdError):
        run()                                                    # CPU tensors: there is no CPU path
