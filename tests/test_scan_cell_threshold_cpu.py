"""CPU: the folded admission threshold of cell_cand_kernel (cell_fold_threshold, csrc/scan_cells.h, exported as
tpq_ivfpq_cell_fold_threshold).  The kernel admits a row when fl(a - q2) >= thr and tests a >= thr2 instead; thr2 must
be the one float for which the two agree for EVERY a.  Checked against a numpy float32 evaluation of fl(a - q2) >= thr
on every float within 8 ulps of thr2 -- the floats next to thr2 on either side are among them, so thr2 is neither too
small nor too large -- over 18 000 sampled (thr, q2) and a list of hand-made ones.  A deliberately wrong folding,
plain fl(thr + q2), goes through the same check and must be caught."""
import ctypes
import functools

import numpy as np

TOP = 0x7f800000  # the image of +inf


def _ord(f):
    """order-preserving integer image of float32 (both zeros -> 0)"""
    b = np.asarray(f, np.float32).view(np.int32).astype(np.int64)
    return np.where(b >= 0, b, -(b & 0x7fffffff))


def _from_ord(o):
    o = np.asarray(o, np.int64)
    return np.where(o >= 0, o, 0x80000000 - o).astype(np.uint32).view(np.float32)


def _ulps(f, n):
    return _from_ord(np.clip(_ord(f) + n, -TOP, TOP))


@functools.lru_cache(maxsize=None)
def _pairs():
    rng = np.random.default_rng(31)
    n = 1500
    f32 = lambda x: np.asarray(x, np.float32)  # noqa: E731
    sign = lambda: rng.choice([-1.0, 1.0], n)  # noqa: E731
    mag = lambda lo, hi: 10.0 ** rng.uniform(lo, hi, n)  # noqa: E731
    thr, q2 = [], []

    def add(t, q):
        thr.append(f32(t))
        q2.append(f32(np.broadcast_to(q, np.shape(t))))
    add(sign() * mag(-30, 30), 0.0)                                   # both signs, q2 = 0
    t = sign() * mag(-10, 20)
    add(t, np.abs(t) * mag(-12, -3))                                  # |thr| >> q2
    q = mag(-10, 20)
    add(sign() * q * mag(-12, -3), q)                                 # q2 >> |thr|
    q = mag(-6, 12)
    add(sign() * q * rng.uniform(0.25, 4.0, n), q)                    # comparable magnitudes
    q = f32(mag(-6, 12))
    add(_ulps(-q, rng.integers(-40, 41, n)), q)                       # thr + q2 cancels: |thr2| << |thr|
    q = f32(mag(-3, 8))
    add(-(q + f32(q * rng.uniform(0.5, 3.0, n))), q)                  # the scan's own: thr ~ -(|q|^2 + |x|^2 - 2 q.x)
    edge = np.ldexp(1.0, rng.integers(-100, 100, n)) * sign()
    add(_ulps(f32(edge), rng.integers(-1, 2, n)), mag(-20, 20))       # thr on / one ulp from a binade edge
    e = rng.integers(-60, 60, n)
    add(_ulps(f32(-np.ldexp(1.0, e)), rng.integers(-1, 2, n)), f32(np.ldexp(1.0, e - rng.integers(0, 26, n))))
    sub = rng.integers(1, 1 << 23, n).astype(np.int64)                # subnormal thr2: a subnormal thr and q2 = 0, ...
    add(_from_ord(sub * rng.choice([-1, 1], n)), 0.0)
    add(_from_ord(sub * rng.choice([-1, 1], n)), _from_ord(rng.integers(0, 1 << 23, n)))  # ... or a subnormal q2
    q = f32(mag(-37, -30))
    add(_ulps(-q, rng.integers(-3, 200, n)), q)                       # ... or what a cancelling thr + q2 leaves
    add(np.full(n // 2, np.inf), mag(-20, 30)[: n // 2])              # thr = +-inf
    add(np.full(n // 2, -np.inf), mag(-20, 30)[: n // 2])
    hand = [(-1.0 + 2.0 ** -24, 1.0), (-1.0, 1.0), (-1.0 - 2.0 ** -23, 1.0), (1.0, 1.0), (3.0e38, 3.0e38),
            (-3.0e38, 3.0e38), (0.0, 0.0), (-0.0, 0.0), (0.0, 1.0), (2.0 ** -149, 0.0), (-2.0 ** -149, 2.0 ** -149),
            (2.0 ** -126, 2.0 ** -149), (3.4e38, 1.0e30), (-3.4e38, 0.0), (np.inf, 0.0), (-np.inf, 0.0), (16777216.0, 1.0),
            (16777218.0, 1.0), (-16777216.0, 3.0)]
    add([h[0] for h in hand], 0.0)
    q2[-1] = f32([h[1] for h in hand])
    thr, q2 = np.concatenate(thr), np.concatenate(q2)
    assert len(thr) >= 10000 and np.isfinite(q2).all() and (q2 >= 0).all() and not np.isnan(thr).any()
    return thr, q2


def _fold_library(thr, q2):
    from torchpq_amd import _lib
    fn = _lib.load().tpq_ivfpq_cell_fold_threshold
    return np.array([fn(ctypes.c_float(t), ctypes.c_float(q)) for t, q in zip(thr.tolist(), q2.tolist())], np.float32)


def _fold_wrong(thr, q2):
    with np.errstate(over="ignore"):
        return (thr + q2).astype(np.float32)


def _mismatches(thr2, thr, q2):
    """per pair: over every float a within 8 ulps of thr2, how often (a >= thr2) and (fl(a - q2) >= thr) differ"""
    assert thr2.dtype == thr.dtype == q2.dtype == np.float32 and not np.isnan(thr2).any()
    a = _from_ord(np.clip(_ord(thr2)[:, None] + np.arange(-8, 9)[None, :], -TOP, TOP))
    with np.errstate(over="ignore", invalid="ignore"):
        kernel = (a - q2[:, None]).astype(np.float32) >= thr[:, None]
    return ((a >= thr2[:, None]) != kernel).sum(1)


def test_folded_threshold_is_the_admission_test_on_every_float_around_it():
    thr, q2 = _pairs()
    thr2 = _fold_library(thr, q2)
    bad = np.nonzero(_mismatches(thr2, thr, q2))[0]
    assert len(bad) == 0, [(thr[i], q2[i], thr2[i]) for i in bad[:5]]
    inf = np.isinf(thr)
    assert np.array_equal(thr2[inf], thr[inf])                        # -inf stays -inf, +inf stays +inf
    sub = (thr2 != 0) & (np.abs(thr2) < np.float32(2.0 ** -126))
    assert sub.sum() >= 1000, "the sample holds too few subnormal folded thresholds"
    far = np.abs(_ord(thr2) - _ord(_fold_wrong(thr, q2))) > 1000
    assert far.sum() >= 100, "the sample holds too few pairs whose fold is far from fl(thr + q2)"


def test_nan_threshold_stays_nan():
    from torchpq_amd import _lib
    fn = _lib.load().tpq_ivfpq_cell_fold_threshold
    assert np.isnan(fn(ctypes.c_float(np.nan), ctypes.c_float(1.0)))


def test_the_check_catches_a_plain_sum():
    """fl(thr + q2) is not the fold: the same check over the same pairs must say so"""
    thr, q2 = _pairs()
    wrong = _mismatches(_fold_wrong(thr, q2), thr, q2)
    assert (wrong > 0).sum() >= 100, (wrong > 0).sum()
    i = np.nonzero((thr == np.float32(-1.0 + 2.0 ** -24)) & (q2 == 1))[0]
    assert len(i) >= 1 and (wrong[i] > 0).all()                       # (the header's example: 2^-24 against 2^-25 + 1 ulp)
