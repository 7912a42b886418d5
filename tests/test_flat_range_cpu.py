"""CPU: the public surface of FlatIndex range search (tpq_flat_range_count / tpq_flat_range_fill, FlatRangeHip,
FlatIndex.range_search), its argument checks and part choice without a GPU, and its oracle (tests/flat_range_oracle.py)
against float64 brute force where fp32 is exact."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import flat_range_oracle as frorc
from conftest import ROOT

#         vectors query a2id  thr   counts n_slots d  nq metric parts stream
COUNT = [None,   None, None, None, None,  100,    8, 1, 0,     1,    None]
#        vectors query a2id  thr   offs  vals  addr  ids   n_slots d  nq metric parts stream
FILL = [None,   None, None, None, None, None, None, None, 100,    8, 1, 0,     1,    None]
NAMES = ("n_slots", "d", "nq", "metric", "parts")


def _dummy(n=1):
    import ctypes as C
    return C.cast((C.c_char * (64 * n))(), C.c_void_p)   # host memory: validation returns before any pointer is read


def test_symbols_wrapper_and_index_surface():
    from torchpq_amd import _lib, kernels
    from torchpq_amd.index import FlatIndex
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in ("tpq_flat_range_segments", "tpq_flat_range_count", "tpq_flat_range_fill"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
        getattr(_lib.load(), name)
    assert "FlatRangeHip" in kernels.__all__ and callable(kernels.FlatRangeHip)
    sig = inspect.signature(kernels.FlatRangeHip.__call__)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("vectors", inspect.Parameter.empty), ("query", inspect.Parameter.empty),
        ("threshold", inspect.Parameter.empty), ("address2id", None), ("distance", "euclidean"), ("n_parts", None)]
    assert kernels.FlatRangeHip().last_n_parts is None
    sig = inspect.signature(FlatIndex.range_search)
    assert [(p.name, p.default) for p in sig.parameters.values()][1:] == [
        ("x", inspect.Parameter.empty), ("threshold", inspect.Parameter.empty), ("return_address", False),
        ("sort", False)]


def test_segments():
    from torchpq_amd import _lib
    seg = _lib.load().tpq_flat_range_segments
    assert seg(1, 1) == 1 and seg(7, 5) == 35 and seg(100_000, 1024) == 102_400_000
    assert seg(3_000_000, 1024) == 3_000_000 * 1024                      # beyond 2^31: a size_t
    assert seg(0, 1) == 0 and seg(-3, 1) == 0 and seg(5, 0) == 0 and seg(5, 1025) == 0 and seg(5, -1) == 0


@pytest.mark.parametrize("entry", ["count", "fill"])
def test_validation_comes_before_any_hip_call(entry):
    from torchpq_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, "tpq_flat_range_" + entry)
    args = COUNT if entry == "count" else FILL
    base = len(args) - 6                                  # position of n_slots
    pos_of = {name: base + i for i, name in enumerate(NAMES)}
    needed = (0, 1, 3, 4) if entry == "count" else (0, 1, 3, 4, 5, 6)
    assert fn(*args) == -1 and "null pointer" in _lib.last_error()
    ok = list(args)
    for pos in needed:
        ok[pos] = _dummy()
    for missing in needed:                                # each required pointer on its own
        a = list(ok)
        a[missing] = None
        assert fn(*a) == -1 and "null pointer" in _lib.last_error(), missing
    for name, bad in (("parts", 0), ("parts", 1025), ("d", 0), ("metric", 2), ("metric", -1), ("nq", -1),
                      ("n_slots", -1)):
        a = list(ok)
        a[pos_of[name]] = bad
        assert fn(*a) == -1, (name, bad)
    if entry == "fill":
        a = list(ok)
        a[7] = _dummy()                                   # out_ids without address2id
        assert fn(*a) == -1 and "address2id" in _lib.last_error()
    a = list(ok)
    a[pos_of["n_slots"]] = (1 << 31) - 1
    assert fn(*a) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
    a[pos_of["d"]] = 0                                    # a bad argument is reported ahead of an unsupported size
    assert fn(*a) == -1
    a = list(ok)
    a[pos_of["nq"]] = 0
    assert fn(*a) == 0                                    # no queries: nothing to do
    a[2] = _dummy()                                       # ... with an id map as well
    assert fn(*a) == 0


def test_wrapper_declines_cpu_tensors_and_a_float64_threshold():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import FlatRangeHip
    vec, q = torch.zeros(4, 100), torch.zeros(4, 2)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        FlatRangeHip()(vec, q, -1.0)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        FlatRangeHip()(vec, q, torch.zeros(2), address2id=torch.zeros(100, dtype=torch.long), distance="inner",
                       n_parts=2)
    with pytest.raises(AssertionError):
        FlatRangeHip()(vec, q, torch.zeros(2, dtype=torch.float64))
    with pytest.raises(AssertionError):
        FlatRangeHip()(vec, q, torch.zeros(3))
    with pytest.raises(AssertionError):
        FlatRangeHip()(vec.double(), q, -1.0)
    with pytest.raises(AssertionError):
        FlatRangeHip()(vec, q, -1.0, address2id=torch.zeros(99, dtype=torch.long))


def test_n_parts_choice():
    from torchpq_amd.kernels.flat import RANGE_BLOCKS_PER_CU, RANGE_ROUNDS, flat_range_parts
    for nq in (1, 100, 128, 129, 1000, 10_000, 32_768, 100_000):
        for n in (0, 1, 255, 256, 257, 5000, 1_000_000, 100_000_000):
            p = flat_range_parts(nq, n, 256)
            assert 1 <= p <= 1024 and p <= max(1, -(-n // 256)), (nq, n, p)
    full = RANGE_ROUNDS * RANGE_BLOCKS_PER_CU * 256
    assert flat_range_parts(1, 1_000_000, 256) == 1024                  # one query group: the cap
    assert flat_range_parts(1000, 1_000_000, 256) == -(-full // 8)      # 8 groups x 256 parts = the wanted grid
    assert flat_range_parts(1000, 1_000_000, 256) * 8 >= full
    assert flat_range_parts(10_000, 1_000_000, 256) == -(-full // 79)
    assert flat_range_parts(1_000_000, 1_000_000, 256) == 1             # the queries alone fill the chip
    assert flat_range_parts(10, 300, 256) == 2                          # fewer chunks than wanted parts: one chunk each
    assert flat_range_parts(10, 256, 256) == 1 and flat_range_parts(10, 0, 256) == 1
    assert flat_range_parts(1, 1_000_000, 8) == 64                      # a small chip


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_oracle_equals_float64_brute_force_on_integer_data(distance):
    """components in -8 ... 8, d = 40: fp32 is exact -- lims, addresses, ids and values must EQUAL float64 brute force,
    with tombstones, with thresholds that tie exactly with stored values, and with +-inf and NaN thresholds"""
    y, x, a2id = frorc.integer_problem()
    nq, n = x.shape[1], y.shape[1]
    vals = frorc.values(y, x, distance)
    exact = frorc.exact_values(y, x, distance)
    assert np.abs(exact).max() < 2 ** 24 and np.array_equal(vals.astype(np.float64), exact)
    live = a2id >= 0
    thr = np.empty(nq, np.float32)
    for q in range(nq):
        row = np.sort(exact[q][live])
        # ON a stored value (the 30th best, the best -- 31 equal vectors tie with slot 40's -- , the worst), between two
        thr[q] = (row[-30], exact[q, 40], row[0], row[-5] + 0.5)[q % 4]
    thr[4], thr[5], thr[6] = np.inf, -np.inf, np.nan
    assert live[40] and live[100:130].sum() > 20
    for a2 in (a2id, None):
        lims, v, a, ids = frorc.range_hits(vals, thr, a2)
        ok = live if a2 is not None else np.ones(n, bool)
        for q in range(nq):
            want = np.nonzero(ok & (exact[q] >= float(thr[q])))[0] if not np.isnan(thr[q]) else np.zeros(0, np.int64)
            seg = slice(lims[q], lims[q + 1])
            assert np.array_equal(a[seg], want) and np.array_equal(v[seg].astype(np.float64), exact[q, want])
            if a2 is not None:
                assert np.array_equal(ids[seg], a2id[want]) and np.all(ids[seg] >= 0)
        hits = np.diff(lims)
        assert hits[4] == 0 and hits[6] == 0 and hits[5] == ok.sum() and lims[-1] == len(a) == len(v)
        assert hits[1] >= 20 and (ids is None) == (a2 is None)
    # exact ties: the threshold of query 1 is the value of the 31 equal vectors; one ulp above loses them all
    lims, v, a, _ = frorc.range_hits(vals, thr, a2id)
    assert np.isin(np.nonzero(live[100:130])[0] + 100, a[lims[1]:lims[2]]).all()
    up = thr.copy()
    up[1] = np.nextafter(thr[1], np.float32(np.inf))
    l2, _, a2_, _ = frorc.range_hits(vals, up, a2id)
    assert not np.isin(np.arange(100, 130), a2_[l2[1]:l2[2]]).any() and 40 not in a2_[l2[1]:l2[2]]
    # a scalar threshold; NaN values are never hits, not even at -inf
    bad = vals.copy()
    bad[2, 7] = np.nan
    lims, v, a, _ = frorc.range_hits(bad, -np.inf)
    assert np.diff(lims).tolist() == [n] * 2 + [n - 1] + [n] * (nq - 3) and not np.isnan(v).any()
    # sort_segments: (value descending, address ascending) inside each query's segment
    lims, v, a, ids = frorc.range_hits(vals, thr, a2id)
    sv, sa, si = frorc.sort_segments(lims, v, a, ids)
    for q in range(nq):
        seg = slice(lims[q], lims[q + 1])
        order = np.lexsort((a[seg], -exact[q, a[seg]]))
        assert np.array_equal(sa[seg], a[seg][order]) and np.array_equal(si[seg], a2id[sa[seg]])
        assert np.array_equal(sv[seg].astype(np.float64), exact[q, sa[seg]])


def test_oracle_returns_plus_zero_and_handles_d1():
    y = np.array([[0.0, -1.0, 2.0, 0.0]], np.float32)
    x = np.array([[-0.0, 3.0]], np.float32)
    ip = frorc.values(y, x, "inner")
    assert not np.signbit(ip[0]).any()                   # -0 * 0, -0 * 2: returned as +0
    assert np.array_equal(ip[1], [0, -3, 6, 0])
    lims, v, a, ids = frorc.range_search(y, x, 0.0, None, "inner")
    assert lims.tolist() == [0, 4, 7] and a.tolist() == [0, 1, 2, 3, 0, 2, 3] and ids is None
    l2 = frorc.values(y, x, "euclidean")
    assert np.array_equal(l2[1], [-9, -16, -1, -9])
