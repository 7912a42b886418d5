"""CPU: IVFPQRIndex's public surface, the new C-ABI symbol, and the re-rank oracle (tests/ivfpqr_oracle.py)
pinned against float64, against the first stage, and against the reference's own decode and metric."""
import importlib.util
import inspect
import os
import re
import warnings

import numpy as np
import pytest

import ivfpqr_oracle as rorc
from conftest import GOLDEN, ROOT, load_golden
from oracle import c_oracle
from oracle import ivfpq_oracle as orc

TOL = 1e-4  # the project's value tolerance (BASELINE.json: rtol = atol = 1e-4)


def test_rerank_symbol_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    assert re.search(r"\btpq_ivfpqr_rerank\s*\(", header)
    assert "tpq_ivfpqr_rerank" in _lib.SIGNATURES
    lib = _lib.load()
    assert hasattr(lib, "tpq_ivfpqr_rerank")
    # validation comes before any HIP call
    args = [None, 10, 8, 8, None, None, None, 32, 1, None, 4, 2, 1, 0, None, None, None, None, None]
    assert lib.tpq_ivfpqr_rerank(*args) == -1 and "null pointer" in _lib.last_error()
    args[8] = 0
    assert lib.tpq_ivfpqr_rerank(*args) == 0  # no queries: nothing to do


def test_index_is_exported_and_aliased():
    import sys
    import torchpq_amd.compat as compat
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    assert "IVFPQRIndex" in index.__all__ and "IVFPQRerankHip" in kernels.__all__
    assert issubclass(index.IVFPQRIndex, index.IVFPQIndex)
    parked = {k: sys.modules.pop(k) for k in list(sys.modules) if k == "torchpq" or k.startswith("torchpq.")}
    compat.install_as_torchpq()
    try:
        from torchpq.index import IVFPQRIndex
        assert IVFPQRIndex is index.IVFPQRIndex
    finally:
        compat.uninstall()
    sys.modules.update(parked)


def test_constructor_signature_and_argument_checks():
    """the reference's parameters in the reference's order (index/IVFPQRIndex.py:8-21) plus a trailing
    rerank_factor; the argument checks come before the device check.  (Containers of this package live on
    the GPU -- BaseContainer refuses device="cpu", as for IVFPQIndex -- so attributes, code_size and the
    _storage shape are checked by the GPU tests.)"""
    from torchpq_amd.index import IVFPQRIndex
    sig = inspect.signature(IVFPQRIndex.__init__)
    got = [(p.name, p.default) for p in list(sig.parameters.values())[1:]]
    assert got == [("d_vector", inspect.Parameter.empty), ("n_subvectors", 8), ("n_subvectors_rerank", 8),
                   ("n_cells", 128), ("use_residual", True), ("initial_size", None), ("expand_step_size", 128),
                   ("expand_mode", "double"), ("distance", "euclidean"), ("device", "cuda:0"), ("verbose", 0),
                   ("rerank_factor", 2)]
    for name in ("vq_codec", "pq_codec", "pq_rerank_codec"):
        for knob in ("max_iter", "n_redo", "tolerance"):
            assert callable(getattr(IVFPQRIndex, f"set_{name}_{knob}"))
    with pytest.raises(AssertionError):
        IVFPQRIndex(32, n_subvectors=8, n_subvectors_rerank=6, device="cpu")    # not a multiple of 4
    with pytest.raises(AssertionError):
        IVFPQRIndex(32, n_subvectors=6, n_subvectors_rerank=8, device="cpu")
    with pytest.raises(AssertionError):
        IVFPQRIndex(40, n_subvectors=8, n_subvectors_rerank=16, device="cpu")   # d % m_r != 0
    with pytest.raises(RuntimeError, match="GPU"):
        IVFPQRIndex(32, n_subvectors=8, n_subvectors_rerank=8, device="cpu")


def _random_case(seed, d, m, m_r, cap, nq, k1, scale=None):
    rng = np.random.default_rng(seed)
    storage = rng.integers(0, 256, ((m + m_r) // 4, cap, 4), dtype=np.uint8)
    cb = rng.standard_normal((m, d // m, 256)).astype(np.float32)
    cb_r = (0.3 * rng.standard_normal((m_r, d // m_r, 256))).astype(np.float32)
    query = rng.standard_normal((d, nq)).astype(np.float32)
    cand = np.stack([rng.choice(cap, k1, replace=False) for _ in range(nq)]).astype(np.int64)
    if scale is not None:   # long vectors: keep |value| near that of the short ones
        cb, cb_r, query = ((a * np.float32(scale)).astype(np.float32) for a in (cb, cb_r, query))
    return storage, cb, cb_r, query, cand


# (d, m, m_r): the first two, then every shape of tests/test_gpu_ivfpqr_edges.py::SLICE_SHAPES (sub-vectors that
# cross the kernel's 16-dimension slices)
ORACLE_SHAPES = [(16, 8, 4), (128, 32, 64), (128, 4, 4), (960, 8, 4), (200, 4, 8), (120, 4, 12), (128, 64, 4),
                 (128, 4, 64), (152, 152, 152)]


def _scale_of(d):
    """the GPU case's scaling: codebooks and query times 1/4 at d = 960"""
    return 0.25 if d >= 960 else None


def _codes_of(storage, lo, hi, address):
    return np.stack([storage[j // 4, address, j % 4] for j in range(lo, hi)])


@pytest.mark.parametrize("d,m,m_r", ORACLE_SHAPES)
@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_oracle_value_against_float64(d, m, m_r, distance):
    storage, cb, cb_r, query, cand = _random_case(d, d, m, m_r, cap=2000, nq=3, k1=150, scale=_scale_of(d))
    if distance == "cosine":
        query = (query / np.linalg.norm(query, axis=0, keepdims=True)).astype(np.float32)
    v = rorc.rerank_values(storage, cb, cb_r, query, cand, True, distance)
    for q in range(query.shape[1]):
        c, c_r = _codes_of(storage, 0, m, cand[q]), _codes_of(storage, m, m + m_r, cand[q])
        recon = orc.pq_decode(cb, c).astype(np.float64) + orc.pq_decode(cb_r, c_r).astype(np.float64)
        x = query[:, q].astype(np.float64)[:, None]
        exact = -((x - recon) ** 2).sum(0) if distance == "euclidean" else (x * recon).sum(0)
        np.testing.assert_allclose(v[q], exact, rtol=TOL, atol=TOL)
    # the non-residual mode is the list scan's value definition on the re-rank rows
    v = rorc.rerank_values(storage, None, cb_r, query, cand, False, distance)
    lut = c_oracle.adc_lut(query, cb_r, distance)
    for q in range(query.shape[1]):
        want = orc.scan_values(np.ascontiguousarray(storage[m // 4:]), lut[:, q], cand[q])
        assert np.array_equal(v[q], want)
        recon = orc.pq_decode(cb_r, _codes_of(storage, m, m + m_r, cand[q])).astype(np.float64)
        x = query[:, q].astype(np.float64)[:, None]
        exact = -((x - recon) ** 2).sum(0) if distance == "euclidean" else (x * recon).sum(0)
        np.testing.assert_allclose(v[q], exact, rtol=TOL, atol=TOL)


@pytest.mark.parametrize("d,m,m_r", ORACLE_SHAPES)
@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_oracle_selection_against_float64(d, m, m_r, distance):
    """residual modes: the oracle's top k (fp32 values, address on ties) is the float64 top k position by position,
    except where the two candidates' float64 values differ by no more than TOL * max(1, |value|) (the rule of
    test_zero_rerank_codebook_keeps_the_first_stage_order); at most 2 % of the positions take the exception"""
    nq, k1, k = 6, 300, 100
    storage, cb, cb_r, query, cand = _random_case(7000 + d + m, d, m, m_r, cap=2000, nq=nq, k1=k1,
                                                  scale=_scale_of(d))
    if distance == "cosine":
        query = (query / np.linalg.norm(query, axis=0, keepdims=True)).astype(np.float32)
    _, adr, _ = rorc.rerank(storage, cb, cb_r, query, cand, k, True, distance)
    excused = 0
    for q in range(nq):
        c, c_r = _codes_of(storage, 0, m, cand[q]), _codes_of(storage, m, m + m_r, cand[q])
        recon = orc.pq_decode(cb, c).astype(np.float64) + orc.pq_decode(cb_r, c_r).astype(np.float64)
        x = query[:, q].astype(np.float64)[:, None]
        exact = -((x - recon) ** 2).sum(0) if distance == "euclidean" else (x * recon).sum(0)
        want = cand[q][np.lexsort((cand[q], -exact))][:k]
        value_of = dict(zip(cand[q].tolist(), exact.tolist()))
        assert np.all(adr[q] >= 0)
        for a, b in zip(adr[q].tolist(), want.tolist()):
            if a != b:
                assert abs(value_of[a] - value_of[b]) <= TOL * max(1.0, abs(value_of[a])), (q, a, b)
                excused += 1
    print(f"d={d} m={m} m_r={m_r} {distance}: {excused} of {nq * k} positions within the tolerance of a tie")
    assert excused <= 0.02 * nq * k, excused


def test_zero_rerank_codebook_keeps_the_first_stage_order():
    """cb_r = 0 with use_residual: the re-ranked value is the first stage's in another summation order, so the
    order is the first stage's except between candidates whose exact values tie to within the tolerance"""
    d, m, m_r = 32, 8, 8
    storage, cb, cb_r, query, cand = _random_case(3, d, m, m_r, cap=3000, nq=4, k1=300)
    cb_r[:] = 0
    lut = c_oracle.adc_lut(query, cb)
    _, adr, _ = rorc.rerank(storage, cb, cb_r, query, cand, 300)
    for q in range(4):
        first = orc.scan_values(np.ascontiguousarray(storage[:m // 4]), lut[:, q], cand[q])
        want = cand[q][np.lexsort((cand[q], -first))]
        recon = orc.pq_decode(cb, _codes_of(storage, 0, m, np.arange(3000))).astype(np.float64)
        exact = -((query[:, q].astype(np.float64)[:, None] - recon) ** 2).sum(0)
        assert sorted(adr[q]) == sorted(want)
        for a, b in zip(adr[q], want):
            assert a == b or abs(exact[a] - exact[b]) <= TOL * max(1.0, abs(exact[a])), (q, a, b)


def test_oracle_selection_ties_missing_and_ids():
    d, m, m_r = 16, 4, 4
    storage, cb, cb_r, query, _ = _random_case(5, d, m, m_r, cap=64, nq=3, k1=4)
    storage[:, 40] = storage[:, 7]            # duplicate code pair at another address: an exact tie
    a2i = np.arange(64, dtype=np.int64) * 10
    cand = np.array([[40, 3, 7, -1, 9], [-1, -1, -1, -1, -1], [64, 2, -5, 1, 2]], dtype=np.int64)
    vals, adr, ids = rorc.rerank(storage, cb, cb_r, query, cand, 5, address2id=a2i)
    assert list(adr[0]).index(7) + 1 == list(adr[0]).index(40) and adr[0, 4] == -1 and vals[0, 4] == -np.inf
    assert np.all(adr[1] == -1) and np.all(ids[1] == -1) and np.all(np.isneginf(vals[1]))
    assert sorted(adr[2][:3]) == [1, 2, 2] and np.all(adr[2][3:] == -1)      # 64 and -5 are no candidates
    assert np.array_equal(ids[adr >= 0], adr[adr >= 0] * 10)
    assert np.all(vals[:, 1:] <= vals[:, :-1])


def _load_generator():
    spec = importlib.util.spec_from_file_location("make_ivfpqr_golden",
                                                  os.path.join(GOLDEN, "make_ivfpqr_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _check_against_reference(fx, ref):
    m, n = fx["codes"].shape
    m_r = fx["codes_r"].shape[0]
    assert np.array_equal(rorc.decode_sum(fx["codebook"], fx["codebook_r"], fx["codes"], fx["codes_r"]),
                          ref["ref_recon"])
    storage = np.zeros(((m + m_r) // 4, n, 4), np.uint8)
    orc.codes_to_storage(np.concatenate([fx["codes"], fx["codes_r"]]), np.arange(n), storage)
    nq = fx["query"].shape[1]
    cand = np.tile(np.arange(n, dtype=np.int64), (nq, 1))
    v = rorc.rerank_values(storage, fx["codebook"], fx["codebook_r"], fx["query"], cand, True, "euclidean")
    np.testing.assert_allclose(v, ref["ref_l2"], rtol=TOL, atol=TOL)
    v = rorc.rerank_values(storage, fx["codebook"], fx["codebook_r"], fx["query_unit"], cand, True, "cosine")
    np.testing.assert_allclose(v, ref["ref_dot"], rtol=TOL, atol=TOL)


def test_oracle_against_the_reference_decode_and_metric():
    """recorded (tests/golden/fx_ivfpqr_pin.npz, written by make_ivfpqr_golden.py) and, where the reference
    tree is present, live"""
    from oracle import _refimport
    fx = load_golden("fx_ivfpqr_pin")
    _check_against_reference(fx, fx)
    if _refimport.available():
        gen = _load_generator()
        inputs = gen.make_inputs()
        for key, value in inputs.items():
            assert np.array_equal(value, fx[key]), key   # the generator still makes the recorded inputs
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _check_against_reference(inputs, gen.reference_results(inputs))
