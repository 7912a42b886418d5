"""GPU: the centroid update of the Lloyd step (update_kernel / finalize_kernel, csrc/lloyd.hip) against the float64 mean
of the step's own labels -- not against ComputeCentroidsHip, which test_gpu_lloyd.py compares it with.

THE BOUND, from lloyd.hip's header.  tpq_lloyd_prepare stores a' = s fl(x - mu) = h + m + rho with fp16 pieces,
|rho| <= 2^-22 |a'| + eta (eta = 2^-13: fp16 subnormals, flushed or not), mu = the fp32 mean of the initial centroids
and s the power of two that puts max |fl(x - mu)| of the sub-problem in [2^13, 2^14), so 1 / s <= R / 2^13 with
R = max |x - mu| over the sub-problem.  update_kernel sums h + m on the fp16 MFMA (exact products 1.0 * piece, fp32 sums)
and finalize_kernel returns mu + (sums / cnt) * (1 / s).  For any mu, mean = mu + (1 / c) sum (x_i - mu), so with
u = 2^-24, D_i = |x_i - mu|, AD = sum of D_i over the cluster, c its size, per element:

    representation      (2^-22 |a'_i| + eta) / s per point     ->  4 u AD / c + eta / s,   eta / s <= 2^-26 R
    one rounding of x - mu                                     ->  u AD / c
    summation of T = 2 c addends and P per-block partial sums  ->  2 (2 c + P) u AD / c   (|h| + |m| <= (1 + 2^-10) |a'|;
                         the factor 2 as in centroid_oracle.bound: the MFMA's internal rounding is not documented)
    sums / cnt rounds once (1 / s and the product with it are exact: a power of two)  ->  u AD / c
    the final mu + ...                                         ->  u |result|

    |new - mean64| <= (1 + 2^-9) ((6 + 4 c + 2 P) u AD / c + 2^-26 R + u |mean64|)

(1 + 2^-9) takes up the second-order terms and the 2^-10 above.  P = the update's blocks per sub-problem (run_update:
2048 / (l * DT) resident waves' worth, DT = ceil(ceil(d / 16) / 2) dimension tiles, at most one per 32-point tile).
mu enters as a magnitude only: the float64 mean of the initial centroids, every D_i widened by 10 u max |centroid| for
what mu_kernel's fp32 tree sum (one value per thread, 8 levels, one division) can differ from it.  For `offset`
(1e4 + N(0, 1)) the bound is an ulp of 1e4 -- u |mean64| = 6e-4 dominates -- not 2 % of the spread.

A flagged sub-problem (non-finite data) is summed by flagged_accum_kernel: raw fp32 values, one global atomic each --
the scalar routes' bound (one addend per point, no partials) and their rule for the non-finite coordinate."""
import numpy as np
import pytest
import torch

import centroid_oracle as O
from test_gpu_lloyd import SHAPES as LLOYD_SHAPES, _data

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = LLOYD_SHAPES + [(1, 64, 8193, 256)]
KINDS = ["gauss", "sift", "offset", "heavy", "clusters"]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def lloyd_partials(l, d, n):
    dt = ((d + 15) // 16 + 1) // 2
    return min(max(1, 2048 // (l * dt)), (n + 31) // 32)


def lloyd_bound(x, cent, labels, k, launched_l=None):
    """(mean64, bound) per element: the module docstring (launched_l: the sub-problems of the call, when x is a slice)"""
    l, d, n = x.shape
    u = O.U
    mu = cent.astype(np.float64).mean(axis=2)
    dmu = 10 * u * np.abs(cent).max(axis=2).astype(np.float64)
    dist = np.abs(x.astype(np.float64) - mu[:, :, None]) + dmu[:, :, None]
    r = dist.max(axis=(1, 2))
    ad, counts = O._sums64(dist, labels, k)
    c = counts[:, None, :].astype(np.float64)
    mean = O.mean64(x, labels, k)
    p = lloyd_partials(launched_l or l, d, n)
    b = (1 + 2.0 ** -9) * ((6 + 4 * c + 2 * p) * u * ad / np.maximum(c, 1) + 2.0 ** -26 * r[:, None, None]
                           + u * np.abs(mean))
    return mean, np.where(c > 0, b, 0.0)


def _inputs(kind, shape, rng):
    l, d, n, k = shape
    x, cent = _data(kind, l, d, n, min(n, k), rng)
    if n < k:       # more centroids than points: repeat points
        cent = np.ascontiguousarray(x[:, :, rng.integers(0, n, k)])
    return x, cent


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "l%d-d%d-n%d-k%d" % s)
def test_lloyd_update_is_the_float64_mean_of_its_own_labels(kind, shape):
    import torchpq_amd.kernels as K
    l, d, n, k = shape
    x, cent = _inputs(kind, shape, np.random.default_rng(O.seed(kind, shape)))
    step = K.LloydStepHip(T(x), T(cent))
    worst = 0.0
    for _ in range(2):                                    # the prepared block keeps serving: same checks twice
        _, lab, new = step(T(cent))
        lab, new = lab.cpu().numpy(), new.cpu().numpy()
        assert lab.min() >= 0 and lab.max() < k
        mean, bnd = lloyd_bound(x, cent, lab, k)
        assert np.isfinite(new).all() and (new[bnd == 0] == 0).all()       # empty clusters exactly 0
        err = np.abs(new.astype(np.float64) - mean)
        ratio = float((err[bnd > 0] / bnd[bnd > 0]).max(initial=0.0))
        worst = max(worst, ratio)
        print(kind, shape, "error / bound", ratio, "max error", float(err.max()), "max bound", float(bnd.max()))
        assert (err <= bnd).all(), (kind, shape, ratio)
    if kind == "offset":
        # decisive: an ulp of 1e4 (2^-10), not the 0.02 that 2e-6 * max |centroid| allowed
        assert bnd.max() < 4 * 2.0 ** -10
    O.record("lloyd", kind, worst)


def test_lloyd_update_flagged_sub_problem_next_to_a_clean_one():
    """one +inf coordinate flags its sub-problem (raw fp32 sums by global atomics): only the owning cluster's element
    of that dimension is non-finite, every other element within the scalar routes' bound; the clean sub-problem next to
    it stays within the bound of the fp16 pieces"""
    import torchpq_amd.kernels as K
    shape = (2, 24, 2000, 64)
    l, d, n, k = shape
    x, cent = _inputs("gauss", shape, np.random.default_rng(O.seed("flagged")))
    clean = x.copy()
    pb, pe, pi = 1, 5, 78
    x[pb, pe, pi] = np.inf
    step = K.LloydStepHip(T(x), T(cent))
    _, lab, new = step(T(cent))
    assert step.rechecked().cpu().numpy()[pb] == n                        # flagged: everything re-checked exactly
    lab, new = lab.cpu().numpy(), new.cpu().numpy()
    assert lab.min() >= 0 and lab.max() < k
    mean, bnd = lloyd_bound(clean[:1], cent[:1], lab[:1], k, launched_l=l)
    assert (np.abs(new[:1].astype(np.float64) - mean) <= bnd).all() and (new[:1][bnd == 0] == 0).all()
    mean, bnd = O.mean_and_bound(clean[1:], lab[1:], k, 1, 0)
    judged = np.ones(mean.shape, bool)
    judged[0, pe, lab[pb, pi]] = False
    got = new[1:]
    assert not np.isfinite(got[0, pe, lab[pb, pi]])
    assert np.isfinite(got[judged]).all() and (got[bnd == 0] == 0).all()
    assert (np.abs(got.astype(np.float64) - mean)[judged] <= bnd[judged]).all()
