"""GPU: ComputeCentroidsHip (tpq_compute_centroids, csrc/centroid_update.hip) against float64 means at the edge shapes
of its three routes -- the bf16 matrix-core route (k <= 256, d >= 32; VEC and non-VEC templates, 1 to 4 tiles in one
block, 2 and 3 blocks per dimension tile), the LDS route (vector and scalar branch, one and several blocks, up to the
k = 2409 that still fits) and the global-atomic route -- with the families of tests/centroid_oracle.py:

  general families  |centroid - mean64| <= bound (the oracle's module docstring), per element;
  exact families    bit for bit: `singletons` (the labelled value itself; every other point carries an out-of-range
                    label, so nothing of those may appear anywhere), `integers_wide`, `integers_small` (float32(S / c));
  every case        empty clusters exactly 0; a second call gives a result that passes the same checks.

Small shapes run every data family under every label family; from 40 000 elements on the data families rotate over the
14 label variants (every data family at least twice per shape, every pair over the table).

TPQ_CENTROID_ERROR_JSON=<path> records the largest error / bound ratio per route and family in that file
(profiles/centroid_update_error.json is such a record; the ratios are records, the bound is the derived one)."""
import numpy as np
import pytest
import torch

import centroid_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# (l, d, n, k)
MFMA_SHAPES = [
    (1, 32, 1, 1), (1, 33, 63, 2), (3, 63, 64, 255), (1, 64, 65, 256), (1, 65, 128, 256), (3, 96, 129, 2),
    (1, 32, 192, 255), (1, 64, 193, 1), (3, 33, 192, 256),
    # 2 and 3 blocks per dimension tile: 64 | 65 tiles in a block
    (1, 64, 8192, 256), (1, 33, 8193, 255), (3, 32, 12288, 2), (1, 96, 12289, 256), (1, 65, 8192, 1),
    (3, 63, 12289, 255),
]
LDS_SHAPES = [
    (1, 1, 3, 7), (3, 15, 4, 257), (1, 16, 4, 7), (3, 16, 4096, 7), (1, 16, 4096, 1024), (1, 17, 4097, 2409),
    (3, 31, 8196, 257), (1, 16, 8196, 2409), (1, 31, 4097, 1024), (1, 33, 4096, 257),
]
GLOBAL_SHAPES = [(1, 16, 255, 2410), (1, 24, 256, 16384), (3, 33, 257, 2410), (1, 16, 5000, 16384), (1, 33, 5000, 2410)]
SHAPES = MFMA_SHAPES + LDS_SHAPES + GLOBAL_SHAPES

DATA_FAMILIES = O.GENERAL + ("integers_wide", "integers_small")
LABEL_VARIANTS = [(name, oor) for name in O.LABELS for oor in (False, True)]


def _offset_view(a, elements):
    """the array on the GPU as a CONTIGUOUS view that starts `elements` elements into its allocation"""
    flat = torch.empty(a.size + elements, dtype={4: torch.float32, 8: torch.int64}[a.itemsize], device=DEV)
    view = flat[elements:].view(*a.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)))
    assert view.is_contiguous() and view.data_ptr() == flat.data_ptr() + elements * a.itemsize
    return view


def _run(x, lab, k, data_offset=0, label_offset=0):
    """two calls of ComputeCentroidsHip on the same device tensors: [first, second] as numpy"""
    import torchpq_amd.kernels as K
    X, Lb = _offset_view(x, data_offset), _offset_view(lab, label_offset)
    if data_offset == 0 and label_offset == 0:
        assert X.data_ptr() % 16 == 0 and Lb.data_ptr() % 16 == 0
    op = K.ComputeCentroidsHip()
    outs = [op(X, Lb, k=k).cpu().numpy() for _ in range(2)]
    assert np.array_equal(X.cpu().numpy().view(np.uint32), x.view(np.uint32))       # inputs untouched (bits: NaN too)
    assert np.array_equal(Lb.cpu().numpy(), lab)
    return outs


def _check_general(outs, x, lab, k, shape, family, tag):
    mean, bnd = O.mean_and_bound(x, lab, k, O.addends_per_point(*shape), O.partials(*shape))
    worst = 0.0
    for out in outs:
        assert out.dtype == np.float32 and np.isfinite(out).all(), tag
        err = np.abs(out.astype(np.float64) - mean)
        assert (out[bnd == 0] == 0).all(), tag                      # empty clusters are exactly 0
        ratio = float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0))
        worst = max(worst, ratio)
        assert (err <= bnd).all(), (tag, "error / bound", ratio)
    O.record(O.route(*shape), family, worst)


def _check_exact(outs, expected, tag):
    for out in outs:
        same = out.view(np.uint32) == expected.view(np.uint32)
        assert same.all(), (tag, int((~same).sum()), "elements differ; first:",
                            out[~same][:3].tolist(), expected[~same][:3].tolist())


def _one(shape, family, lname, oor, data_offset=0, label_offset=0):
    l, d, n, k = shape
    rng = np.random.default_rng(O.seed(shape, family, lname, oor))
    lab = O.make_labels(lname, l, n, k, rng, out_of_range=oor)
    tag = (shape, family, lname, "oor" if oor else "in-range")
    if family in O.GENERAL:
        x = O.make_general(family, l, d, n, rng)
        _check_general(_run(x, lab, k, data_offset, label_offset), x, lab, k, shape, family, tag)
        return
    make = O.make_integers_wide if family == "integers_wide" else O.make_integers_small
    x, lab, expected = make(lab, l, d, n, k, rng)
    _check_exact(_run(x, lab, k, data_offset, label_offset), expected, tag)


def _singletons(shape, data_offset=0, label_offset=0):
    l, d, n, k = shape
    x, lab, expected = O.make_singletons(l, d, n, k, np.random.default_rng(O.seed(shape, "singletons")))
    _check_exact(_run(x, lab, k, data_offset, label_offset), expected, (shape, "singletons"))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "l%d-d%d-n%d-k%d" % s)
def test_centroids_at_the_edge_shapes_of_every_route(shape):
    l, d, n, k = shape
    want = "mfma" if shape in MFMA_SHAPES else "lds" if shape in LDS_SHAPES else "global"
    assert O.route(*shape) == want
    if n >= k:
        _singletons(shape)
    if l * d * n <= 40_000:
        for family in DATA_FAMILIES:
            for lname, oor in LABEL_VARIANTS:
                _one(shape, family, lname, oor)
    else:
        s = SHAPES.index(shape)
        for i, (lname, oor) in enumerate(LABEL_VARIANTS):
            _one(shape, DATA_FAMILIES[(i + s) % len(DATA_FAMILIES)], lname, oor)


@pytest.mark.parametrize("shape,data_offset,label_offset", [
    ((1, 64, 256, 256), 1, 0),      # matrix route, n % 4 == 0, data 4 bytes off a 16-byte boundary: non-VEC
    ((3, 16, 4096, 7), 1, 0),       # LDS route, n % 4 == 0, full dimension tile: data 4 bytes off -> the scalar loop
    ((3, 16, 4096, 7), 0, 1),       # ... labels 8 bytes off
    ((1, 33, 4100, 257), 1, 1),     # both, several dimension tiles
], ids=["mfma-data", "lds-data", "lds-labels", "lds-both"])
def test_centroids_from_views_that_are_not_16_byte_aligned(shape, data_offset, label_offset):
    """a contiguous view with a storage offset passes through .contiguous() unchanged: neither route may take its
    16-byte loads on it (centroid_accum_kernel checks both pointers, the matrix route's launch the data pointer)"""
    _singletons(shape, data_offset, label_offset)
    for family, (lname, oor) in (("gauss", ("uniform", True)), ("offset", ("skewed", False)),
                                 ("integers_wide", ("uniform", False)), ("integers_small", ("gaps_odd", True))):
        _one(shape, family, lname, oor, data_offset, label_offset)


@pytest.mark.parametrize("family", ["gauss", "integers_small"])
@pytest.mark.parametrize("pair", [((1, 31, 4100, 256), (1, 32, 4100, 256)), ((1, 32, 4100, 256), (1, 32, 4100, 257)),
                                  ((3, 31, 193, 256), (3, 32, 193, 256)), ((3, 32, 193, 256), (3, 32, 193, 257))],
                         ids=["d31-32", "k256-257", "d31-32-odd-n", "k256-257-odd-n"])
def test_centroids_across_the_route_boundaries(pair, family):
    """d = 31 | 32 at k = 256 and k = 256 | 257 at d = 32 on identical points and labels: the two sides take different
    routes; both are within the bound of mean64 and, on small integers, bit-equal to each other"""
    a, b = pair
    assert O.route(*a) != O.route(*b) and "mfma" in (O.route(*a), O.route(*b))
    l, d, n, k = b
    rng = np.random.default_rng(O.seed(pair, family))
    lab = O.make_labels("uniform", l, n, 256, rng, out_of_range=True)
    lab = np.where(lab == 256, -1, lab)                               # out of range for k = 256 AND k = 257
    if family == "gauss":
        x = O.make_general("gauss", l, d, n, rng)
    else:
        x, _, _ = O.make_integers_small(lab, l, d, n, 256, rng)
    outs = {}
    for shape in pair:
        xs = np.ascontiguousarray(x[:, :shape[1]])
        outs[shape] = _run(xs, lab, shape[3])
        if family == "gauss":
            _check_general(outs[shape], xs, lab, shape[3], shape, family, (shape, family, "boundary"))
        else:
            _check_exact(outs[shape], O.exact_mean32(xs, lab, shape[3]), (shape, family, "boundary"))
    if family == "integers_small":
        common = tuple(slice(0, min(s, t)) for s, t in zip(outs[a][0].shape, outs[b][0].shape))
        assert np.array_equal(outs[a][0][common].view(np.uint32), outs[b][0][common].view(np.uint32))
        if b[3] == 257:
            assert (outs[b][0][:, :, 256] == 0).all()


@pytest.mark.parametrize("poison", [np.inf, np.nan], ids=["inf", "nan"])
@pytest.mark.parametrize("shape", [(2, 17, 300, 7), (2, 16, 4096, 7), (1, 24, 257, 2410), (2, 40, 200, 9),
                                   (1, 64, 8256, 256)], ids=lambda s: "l%d-d%d-n%d-k%d" % s)
def test_centroids_with_one_non_finite_coordinate(shape, poison):
    """scalar routes: only the owning cluster's element of that dimension is non-finite, every other element within the
    bound; matrix route (0 * inf reaches the clusters of the point's 16-point group, in that dimension only: the kernel
    comment): every element of every OTHER dimension within the bound -- nothing is asserted about the poisoned one --
    and empty clusters are 0 in every dimension"""
    l, d, n, k = shape
    rng = np.random.default_rng(O.seed(shape, "poison"))
    lab = O.make_labels("gaps_even" if k > 1 else "uniform", l, n, k, rng, out_of_range=True)
    x = O.make_general("gauss", l, d, n, rng)
    pb, pe = l - 1, d // 2
    labelled = np.flatnonzero((lab[pb] >= 0) & (lab[pb] < k))
    pi = int(labelled[len(labelled) // 3])                            # a point with a label in range owns the poison
    clean = x.copy()
    x[pb, pe, pi] = poison
    mean, bnd = O.mean_and_bound(clean, lab, k, O.addends_per_point(*shape), O.partials(*shape))
    matrix = O.route(*shape) == "mfma"
    judged = np.ones(mean.shape, bool)
    if matrix:
        judged[pb, pe, :] = False
    else:
        judged[pb, pe, lab[pb, pi]] = False
    for out in _run(x, lab, k):
        assert (out[bnd == 0] == 0).all()                            # empty clusters, the poisoned dimension included
        assert np.isfinite(out[judged]).all()
        assert (np.abs(out.astype(np.float64) - mean)[judged] <= bnd[judged]).all()
        if not matrix:
            assert not np.isfinite(out[pb, pe, lab[pb, pi]])
