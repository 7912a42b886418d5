"""CPU: the group cutting of the filtered exact search (torchpq_amd.kernels.flat.flat_filter_groups): every query in
exactly one group, groups of at most 128 queries of one row, rows outside the filter as -1."""
import numpy as np
import pytest
import torch

import flat_filtered_guarded  # noqa: F401  (registers the guarded case of the new entry points)
from torchpq_amd.kernels.flat import flat_filter_groups


def _check(rows, n_query, n_filters):
    order, begin, grow = (t.numpy() for t in flat_filter_groups(None if rows is None else torch.from_numpy(rows),
                                                                 n_query, n_filters))
    assert order.dtype == begin.dtype == grow.dtype == np.int32
    assert np.array_equal(np.sort(order), np.arange(n_query))            # every query once
    assert begin[0] == 0 and begin[-1] == n_query and len(begin) == len(grow) + 1
    sizes = np.diff(begin)
    assert ((sizes >= 1) & (sizes <= 128)).all()
    assert -(-n_query // 128) <= len(grow) <= n_query or n_query == 0
    want = np.zeros(n_query, np.int64) if rows is None else np.where((rows >= 0) & (rows < n_filters), rows, -1)
    for g in range(len(grow)):
        members = order[begin[g]:begin[g + 1]]
        assert (want[members] == grow[g]).all()                          # one row per group
        assert (np.diff(members) > 0).all()                              # the sort is stable
    return order, begin, grow


@pytest.mark.parametrize("n_query", [0, 1, 128, 129, 300])
def test_no_rows_is_the_identity_in_groups_of_128(n_query):
    order, begin, grow = _check(None, n_query, 3)
    assert np.array_equal(order, np.arange(n_query)) and len(grow) == -(-n_query // 128) and not grow.any()


@pytest.mark.parametrize("n_query", [0, 1, 128, 129, 1000])
@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_rows_are_sorted_and_cut(n_query, dtype):
    rng = np.random.default_rng(n_query)
    rows = rng.integers(-2, 5, n_query).astype(dtype)                    # -2, -1, 3, 4 are outside a filter of 3 rows
    order, begin, grow = _check(rows, n_query, 3)
    assert (np.diff(grow) >= 0).all()
    if n_query == 1000:
        assert (grow == -1).sum() == -(-int(((rows < 0) | (rows >= 3)).sum()) // 128) >= 4   # one run, cut into 128s
    one = _check(np.zeros(n_query, dtype), n_query, 1)
    assert len(one[2]) == -(-n_query // 128)


def test_many_rows_of_one_query_each():
    order, begin, grow = _check(np.arange(500)[::-1].copy(), 500, 500)
    assert len(grow) == 500 and np.array_equal(order, np.arange(500)[::-1]) and np.array_equal(grow, np.arange(500))
