"""CPU: IVFFlatIndex's public surface, the new C-ABI symbols, the byte layout of a stored vector, and the list-scan
oracle (tests/ivfflat_oracle.py) pinned against float64 brute force where fp32 is exact."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ivfflat_oracle as forc
from conftest import ROOT
from oracle import ivfpq_oracle as orc


def _integer_data(seed, d, n, nq):
    """SIFT-like: integer components 0 ... 218"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 219, (d, n)).astype(np.float32), rng.integers(0, 219, (d, nq)).astype(np.float32))


def test_symbols_declared_exported_and_bound():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    for name in ("tpq_ivfflat_scan_topk", "tpq_ivfflat_scan_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % name, header)
        assert name in _lib.SIGNATURES
    assert "acc = acc - t*t" in header and "address ascending" in header
    lib = _lib.load()
    # validation comes before any HIP call
    #       vectors query empty start size npl vals addr n_slots d  nq np k  metric split ws  bytes stream
    args = [None, None, None, None, None, None, None, None, 100, 8, 1, 4, 10, 0, 1, None, 0, None]
    assert lib.tpq_ivfflat_scan_topk(*args) == -1 and "null pointer" in _lib.last_error()
    for pos, bad in ((12, 1025), (12, 0), (9, 0), (13, 2), (14, 0), (11, 0)):
        a = list(args)
        a[pos] = bad
        assert lib.tpq_ivfflat_scan_topk(*a) == -1, (pos, bad)
    a = list(args)
    a[8] = (1 << 31) - 1
    assert lib.tpq_ivfflat_scan_topk(*a) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
    a = list(args)
    a[10] = 0
    assert lib.tpq_ivfflat_scan_topk(*a) == 0  # no queries: nothing to do
    # the workspace holds the parts' lists (64 R keys of 8 bytes, R = 1, 2, 4, 8, 16) and only when there are parts
    assert lib.tpq_ivfflat_scan_workspace_bytes(10, 100, 1) == 0
    assert lib.tpq_ivfflat_scan_workspace_bytes(10, 100, 3) == 10 * 3 * 2 * 64 * 8
    assert lib.tpq_ivfflat_scan_workspace_bytes(7, 1024, 2) == 7 * 2 * 16 * 64 * 8
    assert lib.tpq_ivfflat_scan_workspace_bytes(7, 1, 64) == 7 * 64 * 64 * 8


def test_index_is_exported_and_shares_the_coarse_step():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    from torchpq_amd.container import CellContainer
    from torchpq_amd.index._coarse import CoarseProbeMixin
    assert "IVFFlatIndex" in index.__all__ and "IVFFlatTopkHip" in kernels.__all__
    assert issubclass(index.IVFFlatIndex, CellContainer) and not issubclass(index.IVFFlatIndex, index.IVFPQIndex)
    for cls in (index.IVFFlatIndex, index.IVFPQIndex, index.IVFPQRIndex):
        assert issubclass(cls, CoarseProbeMixin)
        for name in ("probe", "_probe_with_extents", "_probe_prepared"):
            assert getattr(cls, name) is getattr(CoarseProbeMixin, name)
        for name in ("use_smart_probing", "smart_probing_temperature"):
            assert isinstance(getattr(cls, name), property)
    for name in ("train", "add", "remove", "search", "search_cells", "reconstruct", "expand"):
        assert callable(getattr(index.IVFFlatIndex, name))


def test_constructor_signature_and_argument_checks():
    """containers of this package live on the GPU (BaseContainer refuses device="cpu", as for IVFPQIndex): the
    argument checks come first, then the device check; placement and state_dict are checked by the GPU tests"""
    from torchpq_amd.index import IVFFlatIndex
    sig = inspect.signature(IVFFlatIndex.__init__)
    got = [(p.name, p.default) for p in list(sig.parameters.values())[1:]]
    assert got == [("d_vector", inspect.Parameter.empty), ("n_cells", 128), ("initial_size", None),
                   ("expand_step_size", 128), ("expand_mode", "double"), ("distance", "euclidean"),
                   ("device", "cuda:0"), ("verbose", 0)]
    with pytest.raises(AssertionError):
        IVFFlatIndex(0, device="cpu")
    with pytest.raises(AssertionError):
        IVFFlatIndex(8, distance="manhattan", device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        IVFFlatIndex(8, device="cpu")


def test_wrapper_declines_cpu_tensors_and_large_k():
    from torchpq_amd._lib import TorchPQAmdError
    from torchpq_amd.kernels import IVFFlatTopkHip
    vec, q = torch.zeros(4, 100), torch.zeros(4, 2)
    cs, sz, npl = torch.zeros(2, 1, dtype=torch.long), torch.full((2, 1), 10), torch.ones(2, dtype=torch.long)
    with pytest.raises(TorchPQAmdError, match="no CPU fallback"):
        IVFFlatTopkHip()(vec, q, cs, sz, npl, 5)
    with pytest.raises(AssertionError):
        IVFFlatTopkHip()(vec, q, cs, sz, npl, 1025)
    with pytest.raises(AssertionError):
        IVFFlatTopkHip()(vec.double(), q, cs, sz, npl, 5)


@pytest.mark.parametrize("d", [1, 3, 32, 960])
def test_byte_layout_round_trip(d):
    """vectors -> code rows [4 d, n] -> the container's scatter into _storage [d, capacity, 4] -> read as fp32:
    component i of the vector at address a is view(float32)[i, a], whatever its bit pattern"""
    from torchpq_amd.index import IVFFlatIndex
    rng = np.random.default_rng(d)
    n, cap = 37, 101
    bits = rng.integers(0, 1 << 32, (d, n), dtype=np.uint64).astype(np.uint32)   # NaN payloads, -0, denormals too
    x = bits.view(np.float32)
    codes = IVFFlatIndex.vectors_to_codes(torch.from_numpy(x))
    assert codes.shape == (4 * d, n) and codes.dtype == torch.uint8
    assert np.array_equal(codes.numpy(), forc.vectors_to_codes(x))
    for i in (0, d - 1):
        for b in range(4):   # little-endian: row 4 i + b is byte b of component i
            assert np.array_equal(codes.numpy()[4 * i + b], ((bits[i] >> (8 * b)) & 255).astype(np.uint8))
    address = rng.permutation(cap)[:n].astype(np.int64)
    storage = np.zeros((d, cap, 4), np.uint8)
    orc.codes_to_storage(codes.numpy(), address, storage)            # the oracle of tpq_scatter_codes
    got = forc.as_vectors(storage)
    assert got.shape == (d, cap)
    assert np.array_equal(got[:, address].view(np.uint32), bits)
    untouched = np.setdiff1d(np.arange(cap), address)
    assert not got[:, untouched].view(np.uint32).any()
    # the torch view the index hands to the scan, and the way back
    t = torch.from_numpy(storage).view(torch.float32)
    assert t.shape == (d, cap, 1) and t[:, :, 0].is_contiguous()
    assert np.array_equal(t[:, :, 0].numpy().view(np.uint32), got.view(np.uint32))
    back = IVFFlatIndex.codes_to_vectors(codes)
    assert np.array_equal(back.numpy().view(np.uint32), bits)


@pytest.mark.parametrize("distance", ["euclidean", "cosine"])
def test_oracle_equals_float64_brute_force_on_integer_data(distance):
    """d = 32, components 0 ... 218: every partial sum is an integer below 32 * 218^2 < 2^24, so fp32 is exact --
    values and addresses must EQUAL the float64 result"""
    d, n_cells, per_cell, nq, k = 32, 12, 90, 9, 100
    cap = n_cells * per_cell
    base, query = _integer_data(3, d, cap, nq)
    base[:, 100:130] = base[:, 40:41]        # thirty copies of one vector: ties, broken by address
    rng = np.random.default_rng(4)
    sizes = rng.integers(0, per_cell + 1, n_cells).astype(np.int64)
    start = (np.arange(n_cells) * per_cell).astype(np.int64)
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    is_empty[rng.choice(cap, 60, replace=False)] = 1          # tombstones inside the cells
    cells = np.stack([rng.permutation(n_cells)[:5] for _ in range(nq)])
    npl = rng.integers(1, 6, nq).astype(np.int64)
    npl[0] = 5
    v, a = forc.scan_topk(base, query, is_empty, start[cells], sizes[cells], npl, k, distance)
    b64, q64 = base.astype(np.float64), query.astype(np.float64)
    for q in range(nq):
        slots = np.concatenate([np.arange(start[c], start[c] + sizes[c]) for c in cells[q, :npl[q]]])
        slots = slots[is_empty[slots] == 0]
        diff = q64[:, q:q + 1] - b64[:, slots]
        exact = -(diff * diff).sum(0) if distance == "euclidean" else (q64[:, q:q + 1] * b64[:, slots]).sum(0)
        order = np.lexsort((slots, -exact))[:k]
        n = len(order)
        assert np.array_equal(a[q, :n], slots[order]) and np.all(a[q, n:] == -1)
        assert np.array_equal(v[q, :n].astype(np.float64), exact[order]) and np.all(np.isneginf(v[q, n:]))
        assert np.abs(exact).max() < 2 ** 24
    assert np.all(v[:, 1:] <= v[:, :-1])


def test_oracle_probe_rules_ties_and_nan():
    d, cap = 3, 64
    rng = np.random.default_rng(0)
    base = rng.standard_normal((d, cap)).astype(np.float32)
    base[:, 20:30] = base[:, 20:21]                       # ten equal vectors
    query = rng.standard_normal((d, 4)).astype(np.float32)
    query[:, 1] = base[:, 20]
    query[0, 2] = np.nan
    start = np.array([[0, 0, 16, 32]] * 4, np.int64)      # the second probe repeats the first: skipped
    size = np.array([[16, 16, 16, -3]] * 4, np.int64)     # a negative size is an empty cell
    is_empty = np.zeros(cap, np.uint8)
    is_empty[[3, 22]] = 1
    npl = np.array([9, 4, 4, 0], np.int64)                # clamped to [0, 4]
    v, a = forc.scan_topk(base, query, is_empty, start, size, npl, 40)
    live = [s for s in range(32) if s not in (3, 22)]
    assert sorted(a[0][a[0] >= 0]) == live and np.all(a[0, 30:] == -1) and np.all(np.isneginf(v[0, 30:]))
    assert list(a[1, :9]) == [20, 21, 23, 24, 25, 26, 27, 28, 29] and np.all(v[1, :9] == 0)
    assert np.all(a[2] == -1) and np.all(np.isneginf(v[2]))          # every value is NaN: nothing enters
    assert np.all(a[3] == -1)
    v5, a5 = forc.scan_topk(base, query, None, start, size, npl, 5)  # without tombstones, k on the tie
    assert list(a5[1]) == [20, 21, 22, 23, 24]
