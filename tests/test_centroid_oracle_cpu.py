"""CPU: the evidence that tests/centroid_oracle.py's bound and exact families are neither too tight nor blind.

An fp32 numpy emulation of each route's summation (ascending, descending, random order; per-block partials combined
afterwards; three bf16 pieces per point in groups of 16, as the matrix route adds them) stays within HALF of bound()
on every general family and reproduces the exact families bit for bit; three wrong emulations -- the third piece
omitted, an out-of-range point added to cluster 0, counts taken once per dimension tile -- each fail an exact family.
"""
import numpy as np
import pytest

import centroid_oracle as O

L, D, N, K = 2, 5, 1500, 7      # small: the emulation is a Python loop over points

# (name, emulate() arguments, addends per point, partials)
ORDERS = [
    ("ascending", dict(order="ascending"), 1, 1),
    ("descending", dict(order="descending"), 1, 1),
    ("random", dict(order="random"), 1, 1),
    ("partials", dict(order="ascending", blocks=4), 1, 4),
    ("pieces", dict(order="ascending", pieces=3), 3, 1),
    ("pieces_partials", dict(order="random", pieces=3, blocks=3), 3, 3),
]


def _labels(name, oor, seed):
    return O.make_labels(name, L, N, K, np.random.default_rng(seed), out_of_range=oor)


@pytest.mark.parametrize("order", ORDERS, ids=[o[0] for o in ORDERS])
@pytest.mark.parametrize("family", O.GENERAL)
def test_fp32_emulation_stays_within_half_the_bound(family, order):
    _, kw, addends, parts = order
    rng = np.random.default_rng(O.GENERAL.index(family))
    x = O.make_general(family, L, D, N, rng)
    for li, (lname, oor) in enumerate([("uniform", False), ("one_mid", True), ("skewed", True), ("gaps_odd", False)]):
        lab = _labels(lname, oor, 100 + li)
        got = O.emulate(x, lab, K, rng=np.random.default_rng(5), **kw).astype(np.float64)
        ref = O.mean64(x, lab, K)
        bnd = O.bound(x, lab, K, addends, parts)
        err = np.abs(got - ref)
        assert (err <= 0.5 * bnd).all(), (family, lname, float((err / np.maximum(bnd, 1e-300)).max()))
        assert (got[bnd == 0] == 0).all()


def _exact_cases(seed=0):
    """(name, data, labels, expected) of every exact family, the integer ones under two label families"""
    rng = np.random.default_rng(seed)
    x, lab, exp = O.make_singletons(L, D, N, K, rng)
    yield "singletons", x, lab, exp
    for lname, oor in (("uniform", True), ("skewed", False)):
        base = _labels(lname, oor, seed + 7)
        yield ("integers_wide-" + lname,) + O.make_integers_wide(base, L, D, N, K, rng)
        yield ("integers_small-" + lname,) + O.make_integers_small(base, L, D, N, K, rng)


@pytest.mark.parametrize("order", ORDERS, ids=[o[0] for o in ORDERS])
def test_fp32_emulation_reproduces_the_exact_families_bit_for_bit(order):
    _, kw, _, _ = order
    for name, x, lab, exp in _exact_cases():
        got = O.emulate(x, lab, K, rng=np.random.default_rng(5), **kw)
        assert got.dtype == exp.dtype == np.float32
        assert np.array_equal(got.view(np.uint32), exp.view(np.uint32)), name


@pytest.mark.parametrize("wrong,kw", [
    ("third_piece_omitted", dict(pieces=3, drop_third=True)),
    ("out_of_range_point_in_cluster_0", dict(leak_out_of_range=True)),
    ("counts_once_per_dimension_tile", dict(count_per_dtile=2)),
])
def test_wrong_emulations_fail_an_exact_family(wrong, kw):
    failed = [name for name, x, lab, exp in _exact_cases()
              if not np.array_equal(O.emulate(x, lab, K, **kw).view(np.uint32), exp.view(np.uint32))]
    print(wrong, "fails", failed)
    assert failed, wrong
    if wrong == "third_piece_omitted":      # half of the wide integers have a third piece; the small ones none
        assert "singletons" in failed and "integers_wide-uniform" in failed
        assert "integers_small-uniform" not in failed
    if wrong == "out_of_range_point_in_cluster_0":
        assert "singletons" in failed


def test_exact_families_meet_their_preconditions_and_the_third_piece_matters():
    rng = np.random.default_rng(3)
    x, lab, exp = O.make_singletons(1, 3, 40, 40, rng)              # n == k: no out-of-range point at all
    assert ((lab >= 0) & (lab < 40)).all()
    h, m, lo = O.split3_bf16(x)
    assert np.array_equal((h + m).astype(np.float32) + lo, x) and (lo != 0).mean() > 0.9
    xw, _, _ = O.make_integers_wide(_labels("uniform", False, 1), L, D, N, K, rng)
    assert 0.3 < (O.split3_bf16(xw)[2] != 0).mean() < 0.7
    with pytest.raises(AssertionError):
        O.make_singletons(1, 3, 39, 40, rng)


def test_launch_rules_restated():
    """route() and partials() at the shapes the GPU test relies on (centroid_update.hip's launch rules)"""
    assert O.route(1, 31, 100, 256) == "lds" and O.route(1, 32, 100, 256) == "mfma" and O.route(1, 32, 100, 257) == "lds"
    assert O.route(1, 16, 100, 2409) == "lds" and O.route(1, 16, 100, 2410) == "global"
    assert [O.partials(1, 64, n, 256) for n in (1, 8128, 8129, 8193, 12288, 12289)] == [1, 1, 2, 2, 3, 3]
    assert O.partials(4096, 64, 12288, 256) == 1                    # more waves than one round: one block per tile set
    assert [O.partials(1, 16, n, 7) for n in (3, 4096, 4097, 8196)] == [1, 1, 2, 3]
    assert O.partials(1, 16, 5000, 2410) == 0


def test_mean64_ignores_out_of_range_labels_and_zeroes_empty_clusters():
    x = np.arange(12, dtype=np.float32).reshape(1, 2, 6)
    lab = np.array([[0, 2, 2, -1, 3, 2 ** 40]], np.int64)
    m = O.mean64(x, lab, 3)
    assert m.dtype == np.float64 and np.array_equal(m[0], [[0, 0, 1.5], [6, 0, 7.5]])
    assert (O.bound(x, lab, 3, 1, 1)[0, :, 1] == 0).all()
