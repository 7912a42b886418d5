"""CPU: the inputs of test_gpu_scan_rounding_band.py are what that file says they are.

The packed scan selects with a fast fp32 sum of the m table entries and re-evaluates what lies within a band of the
running k-th value with the reference's ascending-j chain; the band is proportional to sum_j max|LUT_j|.  A test of that
band only bites where the ORDER of the fp32 sum decides who is in the top-k.  Here, without any kernel: for the very
inputs of the GPU cases, the oracle's top-k (the chain) against the top-k of a pairwise fp32 sum over the same
candidates (tests_support.pairwise_topk_sets -- a stand-in for "another order", not the kernel's own).

* control rung A = 0 (zero-mean tables, what the rest of the suite draws): no query's k-set differs;
* the rungs marked `disagree=True` in tests_support.BAND_CASES: at least one query's k-set differs;
* every GPU case that asserts the regime "held" (nothing redone) is one of those, so it cannot pass on benign inputs.
"""
import numpy as np
import pytest

import tests_support as S

_LARGE = 64   # queries of a large batch that are examined (the first ones: the full-probe and the repeated-cell rows)


def _queries(case):
    return list(range(min(case["nq"], _LARGE)))


@pytest.mark.parametrize("case", S.BAND_CASES, ids=[c["id"] for c in S.BAND_CASES])
def test_band_case_inputs(case):
    ix = S.band_case_inputs(case)
    lut = ix["lut"]
    assert lut.dtype == np.float32 and lut.shape == (case["m"], case["nq"], 256) and np.isfinite(lut).all()
    if case["A"]:   # the table's bound is what the rung says: sum_j max|LUT_j| >= m A / 2 (mixed: half of the j)
        bound = np.abs(lut).max(axis=2).sum(axis=0)
        assert (bound >= 0.25 * case["m"] * case["A"]).all(), (bound.min(), case["m"] * case["A"])
    differ = S.orders_disagree(ix, lut, case["k"], _queries(case))
    print(f"BAND-CPU {case['id']} queries_differing={len(differ)}/{len(_queries(case))}")
    if case["disagree"] is True:
        assert len(differ) >= 1
    elif case["disagree"] is False:
        assert len(differ) == 0, differ
    if case["expect"] == "held":
        assert case["disagree"] is True, "a case that asserts 'nothing redone' must sit on a rung where the orders disagree"


def test_ladder_of_the_issue_in_isolation():
    """the construction on its own (6 000 candidates, 8 queries, k = 100, each table entry -A + N(0,1)): the chain and
    the pairwise sum pick the same members at A = 0 and different ones from A = 2^14 on (m = 64: from 2^10 on)"""
    for m, A, want in ((64, 0, False), (64, 2 ** 14, True), (64, 2 ** 20, True), (8, 0, False), (8, 2 ** 20, True)):
        rng = np.random.default_rng(m + 7)
        n, nq = 6000, 8
        storage = rng.integers(0, 256, (m // 4, n, 4), dtype=np.uint8)
        case = dict(storage=storage, is_empty=np.zeros(n, np.uint8), cs=np.zeros((nq, 1), np.int64),
                    sz=np.full((nq, 1), n, np.int64), npl=np.ones(nq, np.int64))
        differ = S.orders_disagree(case, S.offset_lut(rng, m, nq, A, "far"), 100)
        assert bool(differ) == want, (m, A, differ)


def test_offset_lut_modes():
    rng = np.random.default_rng(0)
    far = S.offset_lut(rng, 16, 5, 2 ** 14, "far")
    assert abs(far.mean() + 2 ** 14) < 1 and far.std() < 2
    can = S.offset_lut(rng, 16, 5, 2 ** 14, "cancel").astype(np.float64)
    # offsets cancel in pairs: any choice of one entry per j sums to O(sqrt(m)), the bound grows with A
    assert np.abs(can[:, 0, 0].sum()) < 50 and np.abs(can).max(axis=2).sum(axis=0).min() > 16 * 2 ** 14
    assert np.allclose(can[0].mean(), 2 ** 14, atol=1) and np.allclose(can[3].mean(), -2 ** 14 * 1.37, atol=1)
    mix = S.offset_lut(rng, 64, 5, 2 ** 14, "mixed")
    off = np.abs(mix.mean(axis=(1, 2))) > 2 ** 13
    assert off.sum() == 32
    assert {round(float(np.log10(s))) for s in mix[~off].std(axis=(1, 2))} == {-3, 0, 3}
    q, cb = S.offset_query_codebook(rng, 8, 4, 6, 2 ** 14, "euclidean")
    from oracle import c_oracle
    lut = c_oracle.adc_lut(q, cb, "euclidean")
    assert 0.5 * 2 ** 14 < -lut.mean() < 2 * 2 ** 14
    q, cb = S.offset_query_codebook(rng, 8, 4, 6, 2 ** 14, "inner")
    assert 0.3 * 2 ** 14 < np.abs(c_oracle.adc_lut(q, cb, "inner")).mean() < 2 * 2 ** 14
