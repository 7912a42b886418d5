"""CPU: the surface of IVFFlatIndex filtered search -- the index methods, IdFilter.masks -- the filtered oracle
(tests/ivfflat_filtered_oracle.py) against the top-k and range oracles where they must agree, and the conditions on the
inputs of the GPU tests (tests/ivfflat_filtered_cases.py), asserted on the oracle alone."""
import inspect

import numpy as np
import pytest
import torch

import ivfflat_filtered_cases as cases
import ivfflat_filtered_oracle as ffo
import ivfflat_oracle as forc
import ivfflat_range_oracle as rorc


# ---- the surface --------------------------------------------------------------------------------------------------
def test_index_methods_and_signatures():
    from torchpq_amd.index import IVFFlatIndex, IVFPQIndex
    empty = inspect.Parameter.empty
    params = lambda fn: [(p.name, p.default) for p in list(inspect.signature(fn).parameters.values())[1:]]
    assert params(IVFFlatIndex.search_filtered) == params(IVFPQIndex.search_filtered) == [
        ("x", empty), ("k", empty), ("flt", empty), ("filter_of_query", None)]
    assert params(IVFFlatIndex.search_cells_filtered) == [
        ("x", empty), ("cells", empty), ("flt", empty), ("filter_of_query", None), ("n_probe_list", None), ("k", 1),
        ("return_address", False), ("_extents", None)]
    assert params(IVFFlatIndex.id_filter) == params(IVFPQIndex.id_filter) == [("ids", empty)]
    assert params(IVFFlatIndex.range_search_filtered) == [
        ("x", empty), ("threshold", empty), ("flt", empty), ("filter_of_query", None), ("return_address", False),
        ("sort", False)]
    assert params(IVFFlatIndex.range_search_cells_filtered) == [
        ("x", empty), ("cells", empty), ("threshold", empty), ("flt", empty), ("filter_of_query", None),
        ("n_probe_list", None), ("return_address", False), ("_extents", None)]
    # range_search and range_search_cells keep the signatures tests/test_ivfflat_range_cpu.py pins
    assert params(IVFFlatIndex.range_search) == [
        ("x", empty), ("threshold", empty), ("return_address", False), ("sort", False)]


def test_the_filter_adds_no_entry_point():
    """the mask reaches the scan through `is_empty`: the signature table has no symbol for a filtered IVFFlat scan"""
    from torchpq_amd import _lib
    flat = sorted(s for s in _lib.SIGNATURES if "ivfflat" in s)
    assert flat == ["tpq_ivfflat_range_count", "tpq_ivfflat_range_fill", "tpq_ivfflat_range_segments",
                    "tpq_ivfflat_scan_topk", "tpq_ivfflat_scan_workspace_bytes"]


class _Stub:
    """what IdFilter asks of a container"""

    def __init__(self, address2id, is_empty):
        self.device = "cpu"
        self._address2id = torch.from_numpy(address2id)
        self._is_empty = torch.from_numpy(is_empty)
        self._codes_version = 0
        self.asked = 0

    @property
    def capacity(self):
        return self._address2id.shape[0]

    def get_address_by_id(self, ids):
        """the smallest address holding the id, -1 for an unknown one (BaseContainer.get_address_by_id)"""
        self.asked += 1
        a2i = self._address2id
        hit = ids[:, None] == a2i[None, :]
        first = torch.argmax(hit.to(torch.int8), dim=1)
        return torch.where(hit.any(1), first, torch.full_like(first, -1))


def _numpy_masks(address2id, is_empty, id_sets):
    out = np.ones((len(id_sets), len(address2id)), np.uint8)
    for row, ids in zip(out, id_sets):
        for a in range(len(address2id)):
            if is_empty[a] == 0 and address2id[a] >= 0 and address2id[a] in set(ids.tolist()):
                row[a] = 0
    return out


def test_id_filter_masks_against_a_numpy_restatement():
    from torchpq_amd.index._filter import IdFilter
    rng = np.random.default_rng(3)
    cap = 77
    is_empty = (rng.random(cap) < 0.3).astype(np.uint8)
    a2i = np.where(is_empty == 0, rng.permutation(cap) * 3 + 2, -1).astype(np.int64)
    held = a2i[a2i >= 0]
    id_sets = [held, held[::4], np.zeros(0, np.int64), np.array([-1, -5, 10 ** 12, int(held[0]), int(held[0])], np.int64),
               np.concatenate([held[1::2], [1, 4, 7]])]
    stub = _Stub(a2i, is_empty)
    flt = IdFilter(stub, [torch.from_numpy(s) for s in id_sets])
    m = flt.masks()
    assert m.dtype == torch.uint8 and m.shape == (5, cap) and m.is_contiguous()
    want = _numpy_masks(a2i, is_empty, id_sets)
    assert np.array_equal(m.numpy(), want)
    assert np.array_equal(want[0], is_empty) and want[2].all() and (want[3] == 0).sum() == 1
    assert (m.numpy()[:, is_empty != 0] == 1).all()                    # tombstones and free slots stay skipped
    # cached until the container's version or capacity moves
    asked = stub.asked
    assert flt.masks() is m and flt.masks(stub) is m and stub.asked == asked
    with pytest.raises(AssertionError):
        flt.masks(_Stub(a2i, is_empty))                                # another container
    # a remove: the slot becomes a tombstone and the version moves
    gone = int(np.flatnonzero(want[1] == 0)[0])
    is_empty[gone], a2i[gone] = 1, -1
    stub._address2id, stub._is_empty = torch.from_numpy(a2i), torch.from_numpy(is_empty)
    stub._codes_version += 1
    m2 = flt.masks()
    assert m2 is not m and m2[1, gone] == 1 and np.array_equal(m2.numpy(), _numpy_masks(a2i, is_empty, id_sets))
    # growth: more addresses, one of them holding an id the filter named before the container held it
    a2i = np.concatenate([a2i, [-1, 4, -1]]).astype(np.int64)
    is_empty = np.concatenate([is_empty, [1, 0, 1]]).astype(np.uint8)
    stub._address2id, stub._is_empty = torch.from_numpy(a2i), torch.from_numpy(is_empty)
    stub._codes_version += 1
    m3 = flt.masks()
    assert m3.shape == (5, cap + 3) and m3[4, cap + 1] == 0 and m3[:, cap].all() and m3[:4, cap + 1].all()
    assert np.array_equal(m3.numpy(), _numpy_masks(a2i, is_empty, id_sets))


def test_queries_by_row_groups():
    from torchpq_amd.index._filter import queries_by_row
    assert queries_by_row(None, 5, 3, "cpu") == [(0, None)]
    rows = torch.tensor([2, 0, 7, 2, -1, 0, 2], dtype=torch.int32)
    groups = queries_by_row(rows, 7, 3, "cpu")
    assert [(r, q.tolist()) for r, q in groups] == [(0, [1, 5]), (2, [0, 3, 6])]      # rows 7 and -1: no group
    groups = queries_by_row(torch.ones(4, dtype=torch.int32), 4, 3, "cpu")
    assert groups == [(1, None)]                                       # one row for every query: no gather
    assert queries_by_row(torch.full((4,), 3, dtype=torch.int32), 4, 3, "cpu") == []


# ---- the oracle ---------------------------------------------------------------------------------------------------
def test_oracle_filter_rules():
    """a row is a set of extra slots to skip; a row outside [0, n_filters) allows nothing; the all-ones row is the
    unfiltered oracle; the order is (value descending, address ascending) and the pads are (-inf, -1)"""
    rng = np.random.default_rng(1)
    d, cap, nq = 5, 70, 4
    vectors = rng.standard_normal((d, cap)).astype(np.float32)
    vectors[:, 40:50] = vectors[:, 12:13]                                  # eleven equal vectors
    query = rng.standard_normal((d, nq)).astype(np.float32)
    start, size = np.array([[0, 32]] * nq, np.int64), np.array([[32, 38]] * nq, np.int64)
    npl = np.full(nq, 2, np.int64)
    is_empty = np.zeros(cap, np.uint8)
    is_empty[[3, 45]] = 1
    allowed = np.zeros((2, cap), bool)
    allowed[0] = True
    allowed[1, [3, 12, 41, 45, 47, 69]] = True
    rows = np.array([0, 1, 2, -1], np.int32)
    for dist in ("euclidean", "inner"):
        v, a = ffo.scan_topk(vectors, query, is_empty, allowed, rows, start, size, npl, 8, dist)
        ev, ea = forc.scan_topk(vectors, query, is_empty, start, size, npl, 8, dist)
        assert np.array_equal(a[0], ea[0]) and np.array_equal(v[0].view(np.uint32), ev[0].view(np.uint32))
        assert list(a[1][4:]) == [-1] * 4 and sorted(a[1][:4]) == [12, 41, 47, 69] and np.all(np.isneginf(v[1][4:]))
        tied = [i for i in range(4) if a[1][i] in (12, 41, 47)]
        assert [a[1][i] for i in tied] == [12, 41, 47] and len({v[1][i] for i in tied}) == 1    # equal values: by address
        assert np.all(a[2:] == -1) and np.all(np.isneginf(v[2:]))          # no such row
        v0, a0 = ffo.scan_topk(vectors, query, is_empty, allowed, None, start, size, npl, 8, dist)   # None: row 0
        assert np.array_equal(a0, ea) and np.array_equal(v0.view(np.uint32), ev.view(np.uint32))
        # the range form: the same candidates, in scan order
        lims, rv, ra = ffo.range_scan(vectors, query, is_empty, allowed, rows, start, size, npl, -np.inf, dist)
        assert list(np.diff(lims)) == [cap - 2, 4, 0, 0] and list(ra[lims[1]:lims[2]]) == [12, 41, 47, 69]
        el, erv, era = rorc.range_scan(vectors, query, is_empty, start, size, npl, -np.inf, dist)
        assert np.array_equal(ra[:lims[1]], era[:el[1]]) and np.array_equal(rv[:lims[1]].view(np.uint32),
                                                                            erv[:el[1]].view(np.uint32))


def test_the_cases_select_among_values_computed_once_as_the_oracle_does():
    """ivfflat_filtered_cases values the candidates once, without a mask, and lets every row select: that is
    ivfflat_filtered_oracle.scan_topk (per query ivfflat_oracle.scan_topk with is_empty | ~allowed[row])"""
    d, nq, n_probe, distance = 24, 3, 8, "euclidean"
    case = cases.kernel_case(d, nq, n_probe, distance)
    for r in range(len(cases.ROWS)):
        rows = np.full(nq, r, np.int32)
        for k in cases.KS:
            v, a = ffo.scan_topk(case["vectors"], case["query"], case["is_empty"], case["allowed"], rows, case["cs"],
                                 case["sz"], case["npl"], k, cases.metric(distance))
            wv, wa = case["want"][r, k]
            assert np.array_equal(a, wa) and np.array_equal(v.view(np.uint32), wv.view(np.uint32))
    # row 0 allows everything: the unfiltered oracle
    ev, ea = forc.scan_topk(case["vectors"], case["query"], case["is_empty"], case["cs"], case["sz"], case["npl"], 100)
    assert np.array_equal(case["want"][0, 100][1], ea)
    assert np.array_equal(case["want"][0, 100][0].view(np.uint32), ev.view(np.uint32))


def test_walk_model_on_a_hand_made_layout():
    mask = np.zeros(64 * 20, np.uint8)
    tiles = [np.arange(64 * t, 64 * t + 64) for t in range(20)]
    mask[64 * 8:64 * 9] = 1                  # wave 0's second tile: nothing live
    mask[0:40] = 1                           # wave 0's first tile: 24 live
    mask[64 * 16:64 * 16 + 61] = 1           # wave 0's third tile: 3 live, fewer than COMPACT_BELOW: pending
    mask[64:64 + 62] = 1                     # wave 1's first tile: 2 live: pending, drained at the end
    w = cases.walk(mask, tiles)
    assert cases.COMPACT_BELOW == 4
    assert w[0] == dict(part=0, wave=0, skipped=1, full=0, partial=1, sparse=1, takes=0, left=3)
    assert w[1] == dict(part=0, wave=1, skipped=0, full=2, partial=0, sparse=1, takes=0, left=2)
    assert w[4]["full"] == 2 and len(w) == 8 and len(cases.walk(mask, tiles, n_split=3)) == 24
    assert sum(c["skipped"] + c["full"] + c["partial"] + c["sparse"] for c in cases.walk(mask, tiles, n_split=3)) == 20
    # 40 sparse tiles of 3 live slots on one wave: 120 pending in all, one take of 64 on the way, 56 left
    mask = np.ones(64 * 8 * 40, np.uint8)
    tiles = [np.arange(64 * t, 64 * t + 64) for t in range(8 * 40)]
    for t in range(0, 8 * 40, 8):
        mask[64 * t:64 * t + 3] = 0
    w = cases.walk(mask, tiles)
    assert w[0] == dict(part=0, wave=0, skipped=0, full=0, partial=0, sparse=40, takes=1, left=56)
    assert w[1]["skipped"] == 40


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d,nq,n_probe,distance,long", cases.KERNEL_CASES)
def test_gpu_kernel_cases_are_not_vacuous(d, nq, n_probe, distance, long):
    case = cases.kernel_case(d, nq, n_probe, distance, long)
    cap = len(case["is_empty"])
    assert cap % 32 != 0 and case["vectors"].shape == (d, cap) and case["query"].shape == (d, nq)
    cond = cases.conditions(case)
    assert all(cond.values()), cond
    allowed, live, masks = case["allowed"], case["is_empty"] == 0, case["masks"]
    assert allowed.shape == masks.shape == (len(cases.ROWS), cap) and masks.dtype == np.uint8
    assert np.array_equal(masks[0], case["is_empty"]) and masks[1].all()       # ones: the tombstones only; zeros
    start = case["big_start"]
    assert (masks[2] == 0).sum() == 1 and start + 128 <= np.flatnonzero(masks[2] == 0)[0] < start + 192
    assert 0.01 < (masks[3] == 0).sum() / live.sum() < 0.06 and 0.4 < (masks[4] == 0).sum() / live.sum() < 0.6
    # every row allows the tombstones and the free slots, and the mask still skips them; none of them is a result
    assert allowed[:, ~live].all() and masks[:, ~live].all() and (~live).sum() > 25
    for (r, k), (v, a) in case["want"].items():
        got = a[a >= 0]
        assert live[got].all() and allowed[r][got].all() and got.max(initial=0) < cap
        assert np.all(np.isneginf(v[a < 0]))
    assert 300 in case["sz"] and (cases.LONG_CELL in case["sz"] if long else 1500 in case["sz"])
    if nq > 1 and n_probe > 1:
        assert case["cs"][1, 1] == case["cs"][1, 0]                            # one cell listed twice in a row
    if nq >= 100:
        assert (case["npl"] > n_probe).any() and (case["npl"] < n_probe).any() and (case["npl"] == n_probe).any()


def test_the_case_list_covers_the_shapes():
    ds = {c[0] for c in cases.KERNEL_CASES}
    assert ds == {1, 3, 24, 128, 960} and {c[1] for c in cases.KERNEL_CASES} == {1, 3, 1000}
    assert all(c[1] <= 3 for c in cases.KERNEL_CASES if c[0] == 960) and sum(c[4] for c in cases.KERNEL_CASES) >= 3
    for d in ds:
        assert {c[3] for c in cases.KERNEL_CASES if c[0] == d} == {"euclidean", "inner"}
    assert cases.KS == (1, 10, 100, 1024) and cases.SPLITS == (None, 1, 5, 7)
