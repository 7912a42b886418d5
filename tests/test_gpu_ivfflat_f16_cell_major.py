"""GPU: the fp16 lists' cell-major scan (tpq_ivf_flat16_cells_topk, csrc/scan_flat_f16_cells.hip) against
tests/ivfflat_oracle.py on the rounded vectors -- values bit-equal, addresses equal, no query redone unless the case asks
for it -- and IVFFlat16Index with the switch on against the same index with the switch off.  The inputs are those of
tests/test_gpu_ivfflat_cell_major.py, rounded and packed."""
import numpy as np
import pytest
import torch

import guarded_alloc
import ivfflat_f16_cells_guarded
import ivfflat_f16_oracle as f16
import ivfflat_oracle as forc
from test_gpu_ivfflat_cell_major import CAND_CAP, CELL_SIZES, _case
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _run(case, k, distance, first_probe, cand_cap=CAND_CAP, fill=None):
    from torchpq_amd.kernels import IVFFlat16CellTopkHip
    op = IVFFlat16CellTopkHip(first_probe=first_probe, cand_cap=cand_cap)
    op.fill_workspace = fill
    v, a = op(T(f16.pack(case["vectors"]).view(np.int32)), T(case["query"]), T(case["cs"]), T(case["sz"]),
              T(case["npl"]), k, is_empty=T(case["is_empty"]), distance=distance, cells=T(case["cells"]),
              n_cells=len(CELL_SIZES))
    assert op.last_route == "cell_major"
    return N(v), N(a), op


def _check(case, k, distance, first_probe, redone=0, rows=slice(None), **kw):
    v, a, op = _run(case, k, distance, first_probe, **kw)
    ev, ea = forc.scan_topk(f16.rounded(case["vectors"]), case["query"], case["is_empty"], case["cs"], case["sz"],
                            case["npl"], k, distance)
    assert v.shape == ev.shape and v.dtype == np.float32 and a.dtype == np.int64
    assert np.array_equal(a[rows], ea[rows])
    assert np.array_equal(v[rows].view(np.uint32), ev[rows].view(np.uint32))
    assert op.last_redone == redone, op.last_redone      # (the fallback would hide a broken candidate kernel)
    return v, a


# (d, nq, n_probe, first_probe, k, distance): d = 8, 24, 40 end on a slab whose upper k-group is zero-filled
OP_CASES = [
    (8, 3, 4, 1, 1, "euclidean"),
    (8, 1000, 6, 2, 100, "inner"),
    (24, 130, 6, 2, 100, "euclidean"),
    (40, 130, 1, 2, 1, "inner"),
    (128, 130, 6, 4, 256, "euclidean"),
    (128, 1000, 6, 2, 100, "inner"),
    (960, 3, 4, 2, 100, "euclidean"),
]


@pytest.mark.parametrize("d,nq,n_probe,first_probe,k,distance", OP_CASES)
def test_op_against_the_oracle(d, nq, n_probe, first_probe, k, distance):
    case = _case(1000 * d + nq + n_probe, d, nq, n_probe, scale=0.25 if d >= 960 else 1.0)
    v, a = _check(case, k, distance, first_probe)
    assert np.all(v[a < 0] == -np.inf) and np.all(v[:, 1:] <= v[:, :-1])


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_planted_zeros_subnormals_the_largest_half_and_an_overflow(distance):
    """+-0, 2^-24 (an fp16 subnormal: the matrix cores must keep it, or the band needs a term for it), 65504 and a
    component that rounds to inf among the stored halves"""
    case = _case(5, 24, 130, 6)
    rng = np.random.default_rng(9)
    cap = case["vectors"].shape[1]
    case["vectors"][rng.integers(0, 24, 50), rng.integers(0, cap, 50)] = np.tile(
        np.float32([0.0, -0.0, 2.0 ** -24, 65504.0, 1e6]), 10)
    case["vectors"][:, :40] *= np.float32(2.0 ** -22)        # whole vectors of subnormal halves
    assert np.isinf(f16.rounded(case["vectors"])).any()
    _check(case, 100, distance, 2)


@pytest.mark.parametrize("power", [20, -20])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_a_finite_query_is_served_whatever_its_range(distance, power):
    case = _case(128130 + 6, 128, 130, 6)
    case["query"] *= np.float32(2.0 ** power)
    _check(case, 100, distance, 2)


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
@pytest.mark.parametrize("k", [10, 100])
def test_the_band_holds_under_cancellation(k, distance):
    """components 1000 + 0.01 N(0, 1), d = 128: a half near 1000 has a spacing of 0.5, so nearly every stored component
    is 1000 and nearly all values tie; the order is the finish kernel's alone"""
    _check(_case(7 + k, 128, 40, 6, scale=0.01, base=1000.0), k, distance, 2)


def test_overflow_redoes_every_query():
    case = _case(3, 24, 20, 6, dup=False, same=True, full=True)
    _check(case, 10, "euclidean", 1, redone=20, cand_cap=64)


def test_nan_and_inf_queries_are_redone_and_a_dirty_workspace_changes_nothing():
    from torchpq_amd.kernels import IVFFlat16TopkHip
    case = _case(11, 24, 130, 6)
    clean = _check(case, 100, "euclidean", 2, fill=0xFF)
    case["query"][5, 3] = np.nan
    case["query"][7, 100] = np.inf
    keep = np.setdiff1d(np.arange(130), [3, 100])
    v, a = _check(case, 100, "euclidean", 2, redone=2, rows=keep, fill=0xFF)
    assert np.array_equal(a[keep], clean[1][keep])
    ev, ea = IVFFlat16TopkHip()(T(f16.pack(case["vectors"]).view(np.int32)), T(case["query"]), T(case["cs"]),
                                T(case["sz"]), T(case["npl"]), 100, is_empty=T(case["is_empty"]), distance="euclidean")
    for q in (3, 100):
        assert np.array_equal(a[q], N(ea)[q]) and np.array_equal(v[q].view(np.uint32), N(ev)[q].view(np.uint32))


def test_a_d_that_is_no_multiple_of_8_is_declined():
    from torchpq_amd import _lib
    from torchpq_amd.index import IVFFlat16Index
    with pytest.raises(RuntimeError) as err:
        _run(_case(1, 12, 3, 4), 1, "euclidean", 1)
    assert "not supported" in str(err.value) and _lib.last_error().startswith("ivf_flat16_cells: d=12")
    base, queries = _clustered(4, 12, 600, 20)
    idx = IVFFlat16Index(12, n_cells=4, initial_size=64, device=DEV)
    idx.train(T(base))
    idx.add(T(base))
    idx.n_probe, idx.use_cell_major, idx.cell_major_min_batch = 4, True, 1
    idx.search(T(queries), k=10)
    assert idx.last_route == "query_major"


def test_index_with_the_switch_on_equals_the_switch_off():
    from torchpq_amd.index import IVFFlat16Index
    base, queries = _clustered(4, 24, 3000, 300)
    torch.manual_seed(0)
    np.random.seed(0)
    idx = IVFFlat16Index(24, n_cells=16, initial_size=64, device=DEV)
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
    out = guarded_alloc.run_guarded(ivfflat_f16_cells_guarded.build(), monkeypatch=monkeypatch)
    for s, t in zip(out[0x00], out[0xFF]):
        assert s.dtype == t.dtype and s.shape == t.shape and torch.equal(s.view(torch.uint8), t.view(torch.uint8))
