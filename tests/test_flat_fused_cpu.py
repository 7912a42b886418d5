"""CPU: the public surface of the fused exact search (tpq_flat_topk, FlatTopkHip, FlatIndex.use_fused_search), its
argument checks and workspace size without a GPU, and its oracle (tests/flat_oracle.py) against float64 brute force
where fp32 is exact."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flat_oracle as florc
from conftest import ROOT
from oracle import c_oracle

#        vectors query a2id  vals  addr  ids   n_slots d  nq k   metric parts ws    bytes stream
ARGS = [None,   None, None, None, None, None, 100,    8, 1, 10, 0,     1,    None, 0,    None]
N_SLOTS, D, NQ, K, METRIC, PARTS, WS, WS_BYTES = 6, 7, 8, 9, 10, 11, 12, 13


def _dummy(n=1):
    import ctypes as C
    return C.cast((C.c_char * (64 * n))(), C.c_void_p)   # host memory: validation returns before any pointer is read


def test_symbols_wrapper_and_index_surface():
    from torchpq_amd import _lib, kernels
    from torchpq_amd.index import FlatIndex
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in ("tpq_flat_topk", "tpq_flat_topk_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
        getattr(_lib.load(), name)
    assert "FlatTopkHip" in kernels.__all__ and callable(kernels.FlatTopkHip)
    assert FlatIndex.use_fused_search is False and FlatIndex.max_query_batch == 32768
    sig = inspect.signature(FlatIndex.__init__)
    got = [(p.name, p.default) for p in list(sig.parameters.values())[1:]]
    assert got == [("d_vector", inspect.Parameter.empty), ("initial_size", None), ("expand_step_size", 1024),
                   ("expand_mode", "double"), ("device", "cuda:0"), ("distance", "euclidean"), ("verbose", 0)]
    sig = inspect.signature(kernels.FlatTopkHip.__call__)
    assert [p.name for p in sig.parameters.values()] == ["self", "vectors", "query", "k", "address2id", "distance",
                                                         "n_parts"]


def test_validation_comes_before_any_hip_call():
    from torchpq_amd import _lib
    lib = _lib.load()
    assert lib.tpq_flat_topk(*ARGS) == -1 and "null pointer" in _lib.last_error()
    ok = list(ARGS)
    for pos in (0, 1, 3, 4):
        ok[pos] = _dummy()
    for pos, bad in ((K, 0), (K, 1025), (PARTS, 0), (PARTS, 1025), (D, 0), (METRIC, 2), (NQ, -1), (N_SLOTS, -1)):
        a = list(ok)
        a[pos] = bad
        assert lib.tpq_flat_topk(*a) == -1, (pos, bad)
        assert lib.tpq_flat_topk_workspace_bytes(a[NQ], a[K], a[PARTS]) == 0 or pos in (D, METRIC, N_SLOTS)
    a = list(ok)
    a[5] = _dummy()                                   # out_ids without address2id
    assert lib.tpq_flat_topk(*a) == -1 and "address2id" in _lib.last_error()
    a = list(ok)
    a[N_SLOTS] = (1 << 31) - 1
    assert lib.tpq_flat_topk(*a) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
    a = list(ok)
    a[NQ] = 0
    assert lib.tpq_flat_topk(*a) == 0                 # no queries: nothing to do
    # a workspace that is missing or too small
    need = lib.tpq_flat_topk_workspace_bytes(1, 10, 1)
    assert need == 64 * 8
    assert lib.tpq_flat_topk(*ok) == _lib.ERR_WORKSPACE and "workspace" in _lib.last_error()
    a = list(ok)
    a[WS], a[WS_BYTES] = _dummy(8), need - 1
    assert lib.tpq_flat_topk(*a) == _lib.ERR_WORKSPACE


def test_workspace_is_a_function_of_nq_k_parts_only():
    from torchpq_amd import _lib
    ws = _lib.load().tpq_flat_topk_workspace_bytes
    assert ws(0, 10, 1) == 0 and ws(-3, 10, 1) == 0
    assert ws(10, 100, 3) == 10 * 3 * 2 * 64 * 8 and ws(7, 1024, 2) == 7 * 2 * 16 * 64 * 8
    for nq, k, parts in ((1, 1, 1), (33, 64, 7), (1000, 100, 32), (5, 1000, 1000)):
        base = ws(nq, k, parts)
        assert base > 0
        assert ws(nq + 1, k, parts) >= base and ws(nq, min(k + 1, 1024), parts) >= base
        assert ws(nq, min(2 * k, 1024), parts) >= base and ws(nq, k, parts + 1) >= base
    last = 0
    for k in range(1, 1025):
        assert ws(3, k, 2) >= last
        last = ws(3, k, 2)
    # the matrix this route replaces: 1 000 queries x 1 M slots of fp32
    assert ws(1000, 100, 32) < (1000 * 1_000_000 * 4) // 10


def test_n_parts_choice():
    from torchpq_amd.kernels.flat import flat_parts
    for nq in (1, 100, 128, 129, 1000, 10_000, 32_768, 100_000):
        for n in (1, 255, 256, 5000, 1_000_000, 100_000_000):
            p = flat_parts(nq, n, 256)
            assert 1 <= p <= 1024 and p <= max(1, -(-n // 256)), (nq, n, p)
    assert flat_parts(1000, 1_000_000, 256) * 8 in range(218, 513)     # one or two rounds of workgroups over the CUs
    assert flat_parts(100_000, 1_000_000, 256) == 1                     # the queries alone fill the chip
    assert flat_parts(10, 300, 256) == 2                                # never more parts than chunks


def test_oracle_values_are_the_pinned_chains():
    """d = 37, nq = 9, n = 300: for "euclidean" the block-wise adc_lut equals c_oracle.coarse_sims bit for bit, and its
    row maxima are those of c_oracle.max_sim in both metrics"""
    rng = np.random.default_rng(0)
    d, nq, n = 37, 9, 300
    y = rng.standard_normal((d, n)).astype(np.float32)
    x = rng.standard_normal((d, nq)).astype(np.float32)
    l2 = florc.values(y, x, "euclidean")
    assert np.array_equal(l2.view(np.uint32), c_oracle.coarse_sims(x, y).view(np.uint32))
    ip = florc.values(y, x, "inner")
    for vals, dist, numerics in ((ip, "inner", "direct"), (l2, "euclidean", "expanded")):
        mv, mi = c_oracle.max_sim(x[None], y[None], dist, numerics)
        assert np.array_equal(vals.max(1).view(np.uint32), mv[0].view(np.uint32))
        assert np.array_equal(vals.argmax(1), mi[0])
    # d = 1: the NumPy form
    y1, x1 = y[:1], x[:1]
    for dist in ("euclidean", "inner"):
        assert np.array_equal(florc.values_d1(y1, x1, dist).view(np.uint32), florc.values(y1, x1, dist).view(np.uint32))


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_oracle_equals_float64_brute_force_on_integer_data(distance):
    """components in -3 ... 3, d = 16: every partial sum is a small integer, fp32 is exact -- values and addresses
    must EQUAL the float64 result, ties (many: the values are small integers) broken by address"""
    rng = np.random.default_rng(5)
    d, n, nq, k = 16, 700, 11, 100
    y = rng.integers(-3, 4, (d, n)).astype(np.float32)
    x = rng.integers(-3, 4, (d, nq)).astype(np.float32)
    y[:, 100:130] = y[:, 40:41]
    a2id = np.arange(n, dtype=np.int64) * 3 + 1
    a2id[rng.choice(n, 80, replace=False)] = -1
    v, a, ids = florc.search(y, x, k, a2id, distance)
    y64, x64 = y.astype(np.float64), x.astype(np.float64)
    slots = np.nonzero(a2id >= 0)[0]
    for q in range(nq):
        if distance == "euclidean":
            exact = -((x64[:, q:q + 1] - y64[:, slots]) ** 2).sum(0)
        else:
            exact = (x64[:, q:q + 1] * y64[:, slots]).sum(0)
        order = np.lexsort((slots, -exact))[:k]
        assert np.array_equal(a[q], slots[order]) and np.array_equal(ids[q], a2id[slots[order]])
        assert np.array_equal(v[q].astype(np.float64), exact[order])
        assert len(np.unique(exact[order])) < k // 2          # the order inside the ties is checked
    # fewer live slots than k; NaN and -inf values
    a2id[:] = -1
    a2id[[5, 9, 300]] = [50, 90, 3000]
    y[0, 9] = np.nan
    y[:, 300] = 1e30
    v, a, ids = florc.search(y, x, 4, a2id, distance)
    if distance == "euclidean":
        assert np.all(a == [5, 300, -1, -1]) and np.all(ids == [50, 3000, -1, -1]) and np.all(np.isneginf(v[:, 1:]))
    else:
        assert np.all(a[:, 2:] == -1) and np.all(np.sort(a[:, :2], 1) == [5, 300]) and not np.isnan(v).any()


def test_wrapper_declines_cpu_tensors_and_bad_arguments():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import FlatTopkHip
    vec, q = torch.zeros(4, 100), torch.zeros(4, 2)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        FlatTopkHip()(vec, q, 5)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        FlatTopkHip()(vec, q, 5, address2id=torch.zeros(100, dtype=torch.long), distance="inner", n_parts=2)
    with pytest.raises(AssertionError):
        FlatTopkHip()(vec, q, 1025)
    with pytest.raises(AssertionError):
        FlatTopkHip()(vec.double(), q, 5)
    with pytest.raises(AssertionError):
        FlatTopkHip()(vec, q, 5, address2id=torch.zeros(99, dtype=torch.long))
