"""GPU: tpq_flat_topk (FlatTopkHip) against tests/flat_oracle.py -- addresses equal, values equal as uint32 -- at the
tile, chunk, wave, block and list-register edges, for every way of cutting the slots into parts, with tombstones,
ties, the admission worst case, non-finite values and addresses beyond 2^24.  Standard-normal scale: no subnormal
products (MFMA subnormal handling is not pinned)."""
import numpy as np
import pytest
import torch

import flat_oracle as florc
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu

_OP = []


def _op():
    from torchpq_amd.kernels import FlatTopkHip
    if not _OP:
        _OP.append(FlatTopkHip())
    return _OP[0]


def _data(seed, d, n, nq, scale=1.0):
    rng = np.random.default_rng(seed)
    return ((scale * rng.standard_normal((d, n))).astype(np.float32),
            (scale * rng.standard_normal((d, nq))).astype(np.float32))


def _run(vectors, query, k, a2id=None, distance="euclidean", n_parts=None):
    v, a, ids = _op()(T(vectors), T(query), k, address2id=None if a2id is None else T(a2id), distance=distance,
                      n_parts=n_parts)
    torch.cuda.synchronize()
    assert (ids is None) == (a2id is None)
    assert v.shape == a.shape == (query.shape[1], k) and v.dtype == torch.float32 and a.dtype == torch.int64
    return N(v), N(a), None if ids is None else N(ids)


def _check(got, want, what=""):
    (v, a, ids), (ev, ea, eids) = got, want
    assert np.array_equal(a, ea), (what, np.argwhere(a != ea)[:5])
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32)), (what, np.argwhere(v != ev)[:5])
    if eids is not None:
        assert np.array_equal(ids, eids), what


# (d, n_slots, nq, k, n_parts, distance): d at the 16-row slab edge and odd against the 2-wide MFMA k-step; n_slots at
# the tile (32) and chunk (256) edges; nq at the half-wave, wave and block edges; k at the list-register edges and
# above the live slots; n_parts beyond the number of chunks (empty parts)
CASES = [
    (1, 1, 1, 1, None, "euclidean"), (1, 31, 33, 63, 1, "inner"), (2, 32, 31, 64, 2, "euclidean"),
    (2, 255, 32, 65, 3, "inner"), (15, 256, 127, 100, 7, "euclidean"), (15, 257, 128, 128, 64, "inner"),
    (16, 513, 129, 129, None, "euclidean"), (16, 5000, 300, 1000, 1, "inner"), (17, 5000, 1, 1024, 2, "euclidean"),
    (17, 1, 300, 1, 3, "inner"), (33, 31, 129, 63, 7, "euclidean"), (33, 32, 128, 64, 64, "inner"),
    (128, 255, 127, 65, None, "euclidean"), (128, 256, 33, 100, 1, "inner"), (200, 257, 32, 128, 2, "euclidean"),
    (200, 513, 31, 129, 3, "inner"), (1, 5000, 1, 1000, 7, "euclidean"), (2, 5000, 31, 1024, 64, "inner"),
    (15, 513, 32, 1, None, "inner"), (16, 257, 33, 63, 1, "euclidean"), (17, 256, 127, 64, 2, "inner"),
    (33, 255, 128, 65, 3, "euclidean"), (128, 32, 129, 100, 7, "inner"), (200, 31, 300, 128, 64, "euclidean"),
    (128, 5000, 300, 100, None, "euclidean"), (128, 5000, 129, 129, 3, "inner"), (200, 5000, 33, 1024, 7, "inner"),
    (33, 5000, 128, 1000, 64, "euclidean"), (17, 513, 127, 1024, 1, "inner"), (16, 1, 1, 128, 64, "euclidean"),
    (15, 5000, 300, 64, 2, "euclidean"), (2, 513, 300, 65, None, "inner"), (1, 257, 129, 63, 3, "euclidean"),
    (1, 256, 128, 1, 7, "inner"), (33, 257, 1, 100, 2, "euclidean"), (200, 256, 31, 1000, None, "inner"),
    (128, 513, 32, 129, 64, "euclidean"), (16, 255, 33, 128, 7, "inner"), (17, 32, 127, 65, None, "euclidean"),
    (15, 31, 128, 1024, 1, "inner"),
]


@pytest.mark.parametrize("d,n,nq,k,n_parts,distance", CASES)
def test_kernel_equals_oracle(d, n, nq, k, n_parts, distance):
    vectors, query = _data(d * 1000 + n + nq, d, n, nq)
    rng = np.random.default_rng(k)
    a2id = None
    if (d + n + nq + k) % 2:   # every other case carries an id map with some tombstones
        a2id = rng.permutation(n).astype(np.int64) + 7
        a2id[rng.random(n) < 0.1] = -1
    _check(_run(vectors, query, k, a2id, distance, n_parts), florc.search(vectors, query, k, a2id, distance),
           (d, n, nq, k, n_parts))


@pytest.fixture(scope="module")
def shared():
    """one problem and its oracle values for the tests below: 1 300 slots (6 chunks, the last partial), 70 queries"""
    d, n, nq = 24, 1300, 70
    vectors, query = _data(77, d, n, nq)
    vals = {dist: florc.values(vectors, query, dist) for dist in ("euclidean", "inner")}
    for v in vals.values():
        v.setflags(write=False)
    return dict(d=d, n=n, nq=nq, vectors=vectors, query=query, vals=vals)


def test_same_bits_for_every_n_parts(shared):
    a2id = np.arange(shared["n"], dtype=np.int64)
    a2id[::7] = -1
    want = florc.topk(shared["vals"]["euclidean"], 100, a2id)
    for n_parts in (1, 3, 8):
        _check(_run(shared["vectors"], shared["query"], 100, a2id, "euclidean", n_parts), want, n_parts)


@pytest.mark.parametrize("which", ["every_other", "one_chunk", "the_top_k", "all", "none"])
def test_tombstones(shared, which):
    n, k = shared["n"], 50
    vals = shared["vals"]["inner"]
    a2id = np.arange(n, dtype=np.int64) + 100
    if which == "every_other":
        a2id[::2] = -1
    elif which == "one_chunk":
        a2id[256:512] = -1
    elif which == "the_top_k":
        _, top, _ = florc.topk(vals[:1], k, None)          # exactly the first query's true top-k
        a2id[top[0]] = -1
    elif which == "all":
        a2id[:] = -1
    else:
        a2id = None
    got = _run(shared["vectors"], shared["query"], k, a2id, "inner", 3)
    _check(got, florc.topk(vals, k, a2id), which)
    if which == "all":
        assert np.all(got[1] == -1) and np.all(got[2] == -1) and np.all(np.isneginf(got[0]))
    if which == "the_top_k":
        assert not np.isin(got[1][0], top[0]).any()


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
def test_ties_copies_of_five_vectors(distance):
    """a third of the slots hold one of five vectors and one query equals one of them (test_gpu_ivfflat._case)"""
    d, n, nq = 19, 2100, 40
    vectors, query = _data(3, d, n, nq)
    rng = np.random.default_rng(4)
    src = rng.choice(n, 5, replace=False)
    dst = rng.choice(n, n // 3, replace=False)
    vectors[:, dst] = vectors[:, src[rng.integers(0, 5, len(dst))]]
    query[:, 0] = vectors[:, src[0]]
    for k, n_parts in ((10, None), (100, 2), (700, 5)):
        _check(_run(vectors, query, k, None, distance, n_parts), florc.search(vectors, query, k, None, distance), k)


def test_ties_integer_data_many_way_tie_at_kth_place():
    rng = np.random.default_rng(8)
    d, n, nq = 4, 3000, 50
    vectors = rng.integers(-2, 3, (d, n)).astype(np.float32)
    query = rng.integers(-2, 3, (d, nq)).astype(np.float32)
    for distance in ("euclidean", "inner"):
        want = florc.search(vectors, query, 100, None, distance)
        more = florc.search(vectors, query, 110, None, distance)
        assert (more[0][:, 99] == more[0][:, 109]).mean() > 0.7     # the k-th place sits inside a many-way tie
        for n_parts in (1, 4):
            _check(_run(vectors, query, 100, None, distance, n_parts), want, (distance, n_parts))


def test_ties_copies_across_chunk_and_part_boundaries():
    d, n, nq, k = 8, 1024, 5, 30
    vectors, query = _data(11, d, n, nq)
    vectors[:, 250:262] = query[:, :1]          # chunk boundary at 256
    vectors[:, 506:518] = query[:, :1]          # chunk boundary at 512 = the part boundary for n_parts = 2
    want = florc.search(vectors, query, k)
    assert list(want[1][0, :24]) == list(range(250, 262)) + list(range(506, 518))
    for n_parts in (1, 2, 4):
        _check(_run(vectors, query, k, None, "euclidean", n_parts), want, n_parts)


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_admission_worst_case(order):
    """every slot better than all before it: every value is pushed and the fold path runs hundreds of times (and the
    reverse: nothing after the first k is admitted)"""
    d, n, nq, k = 3, 5000, 40, 100
    rng = np.random.default_rng(21)
    vectors = np.zeros((d, n), np.float32)
    col = np.sort(rng.standard_normal(n).astype(np.float32))
    vectors[0] = col if order == "ascending" else col[::-1]
    query = np.zeros((d, nq), np.float32)
    query[0] = 0.5 + rng.random(nq).astype(np.float32)         # positive: value order = order of the component
    want = florc.search(vectors, query, k, None, "inner")
    for n_parts in (1, 3):
        _check(_run(vectors, query, k, None, "inner", n_parts), want, n_parts)


def test_non_finite_values(shared):
    d, n = shared["d"], 300
    vectors = shared["vectors"][:, :n].copy()
    query = shared["query"][:, :40].copy()
    clean = florc.search(vectors, query, 20)
    # a stored NaN never appears, the rows are those of the other slots
    nan_slot = int(clean[1][0, 0])
    vectors[3, nan_slot] = np.nan
    got = _run(vectors, query, 20, None, "euclidean", 2)
    _check(got, florc.search(vectors, query, 20), "nan slot")
    assert not (got[1] == nan_slot).any() and not np.isnan(got[0]).any()
    a2id_but = np.arange(n, dtype=np.int64)
    a2id_but[nan_slot] = -1
    _check((got[0], got[1], None), florc.search(shared["vectors"][:, :n], query, 20, a2id_but)[:2] + (None,), "as if dead")
    # a stored vector of 1e30 components: value -inf for L2; returned, with its address, only when fewer than k
    # finite candidates exist, ahead of the pads
    vectors = shared["vectors"][:, :50].copy()
    vectors[:, 17] = 1e30
    got = _run(vectors, query, 10, None, "euclidean", 1)
    _check(got, florc.search(vectors, query, 10), "inf, k small")
    assert not (got[1] == 17).any()
    got = _run(vectors, query, 64, None, "euclidean", 1)
    _check(got, florc.search(vectors, query, 64), "inf, k large")
    assert np.all(got[1][:, 49] == 17) and np.all(np.isneginf(got[0][:, 49:])) and np.all(got[1][:, 50:] == -1)
    # a query with a NaN component: the other rows are bit-equal to a run without it
    vectors = shared["vectors"][:, :n]
    bad = query.copy()
    bad[5, 7] = np.nan
    got = _run(vectors, bad, 20, None, "euclidean", 2)
    keep = np.arange(40) != 7
    _check(tuple(x[keep] for x in got[:2]) + (None,), tuple(x[keep] for x in clean[:2]) + (None,), "nan query")


def test_addresses_beyond_2_pow_24():
    n, nq, k = (1 << 24) + 300, 3, 10
    rng = np.random.default_rng(2)
    vectors = (10.0 + rng.standard_normal((1, n))).astype(np.float32)
    query = np.array([[-1.0, -2.0, -2.5]], np.float32)
    vectors[0, -7:] = [-1.0, -2.0, -2.5, -1.0, -1.001, -2.002, -2.499]     # the best slots sit at the far end
    want = florc.topk(florc.values_d1(vectors, query), k)
    assert (want[1][:, :3] >= (1 << 24)).all()
    _check(_run(vectors, query, k), want)
