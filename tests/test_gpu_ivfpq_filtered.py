"""GPU: IVFPQIndex filtered search (tpq_ivfpq_scan_filtered_topk / _residual_topk, tpq_slot_filter_build) against
tests/ivfpq_filtered_oracle.py -- addresses equal, value bits equal, ids equal -- on the inputs of
tests/ivfpq_filtered_cases.py (whose conditions tests/test_ivfpq_filtered_cpu.py asserts), against the unfiltered exact
scan where the two must agree, and the index end to end."""
import numpy as np
import pytest
import torch

import ivfpq_filtered_cases as cases
import ivfpq_filtered_oracle as forc
from oracle import c_oracle
from oracle import ivfpq_oracle as orc
from tests_support import DEV, N, T, _clustered

pytestmark = pytest.mark.gpu


def _gpu(case):
    """the case's arrays on the GPU, uploaded once; an address2id that no result can take for an address"""
    if "gpu" not in case:
        g = {k: T(v) for k, v in case.items() if isinstance(v, np.ndarray) and k not in ("allowed", "bits")}
        g["bits"] = T(case["bits"].view(np.int32))
        case["a2i"] = np.where(case["is_empty"] == 0, 3 * np.arange(len(case["is_empty"])) + 11, -1).astype(np.int64)
        g["a2i"] = T(case["a2i"])
        g["runs"] = [None if r is None else T(r) for r in case["runs"]]
        case["gpu"] = g
    return case["gpu"]


def _same(case, got, want, k):
    v, a, i = got
    ev, ea = want
    nq = case["cs"].shape[0]
    assert v.dtype == torch.float32 and a.dtype == i.dtype == torch.int64 and v.shape == a.shape == i.shape == (nq, k)
    v, a, i = N(v), N(a), N(i)
    assert np.array_equal(a, ea)
    assert np.array_equal(v.view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(i, np.where(ea >= 0, case["a2i"][np.maximum(ea, 0)], -1))


def _run_plain(case, table, metric, run, k, n_split=None, op=None):
    from torchpq_amd.kernels import IVFPQFilteredTopkHip
    g = _gpu(case)
    op = op or IVFPQFilteredTopkHip(m=case["storage"].shape[0] * 4)
    tables = dict(precomputed=g["lut"]) if table == "materialised" else dict(query=g["query"], codebook=g["codebook"])
    return op(g["storage"], g["cs"], g["sz"], g["npl"], k, g["bits"], g["runs"][run], distance=metric,
              is_empty=g["is_empty"], address2id=g["a2i"], n_split=n_split, **tables)


def _run_residual(case, tables, run, k, op=None):
    from torchpq_amd.kernels import IVFPQFilteredTopkHip
    g = _gpu(case)
    op = op or IVFPQFilteredTopkHip(m=case["storage"].shape[0] * 4)
    if tables == "full":
        kw = dict(full=g["full"])
    elif tables == "part1":
        kw = dict(part1=g["part1"], part2=g["part2"], cells=g["cells"])
    else:
        kw = dict(query=g["query"], codebook=g["codebook"], part2=g["part2"], cells=g["cells"])
    return op.residual(g["storage"], g["base_sims"], g["cs"], g["sz"], g["npl"], k, g["bits"], g["runs"][run],
                       is_empty=g["is_empty"], address2id=g["a2i"], **kw)


@pytest.mark.parametrize("m,ds,table,nq,n_probe,metric", cases.PLAIN_CASES)
def test_plain_against_the_oracle(m, ds, table, nq, n_probe, metric):
    """every run of filter rows (the last one passes no filter_of_query), every k and every n_split give the oracle's
    addresses, value bits and ids, hence the same as every other split"""
    from torchpq_amd.kernels import IVFPQFilteredTopkHip
    case = cases.plain_case(m, ds, table, nq, n_probe, metric)
    op = IVFPQFilteredTopkHip(m=m)
    for run in range(len(case["runs"])):
        for k in cases.KS:
            for n_split in cases.SPLITS:
                got = _run_plain(case, table, metric, run, k, n_split, op)
                _same(case, got, case["want"][run, k], k)
                if n_split is None:   # the wrapper splits a small batch over several workgroups, leaves a large one whole
                    assert (op.last_n_split > 1) if nq <= 3 else (op.last_n_split == 1), op.last_n_split
                else:
                    assert op.last_n_split == n_split
        filled = (case["want"][run, 1000][1] >= 0).sum(1)
        print(f"m={m} nq={nq} run {run}: candidates per query min {filled.min()} max {filled.max()}")


@pytest.mark.parametrize("m,ds,tables,nq,n_probe", cases.RESIDUAL_CASES)
def test_residual_against_the_oracle(m, ds, tables, nq, n_probe):
    case = cases.residual_case(m, ds, tables, nq, n_probe)
    for run in range(len(case["runs"])):
        for k in cases.KS:
            _same(case, _run_residual(case, tables, run, k), case["want"][run, k], k)


def test_both_residual_table_forms_give_the_same_bits():
    """part1 given and part1 built in the workgroup, on one case"""
    case = cases.residual_case(64, 2, "built", 3, 8)
    for run in (0, 3, len(case["runs"]) - 1):
        for k in (10, 1000):
            for tables in ("part1", "built"):
                _same(case, _run_residual(case, tables, run, k), case["want"][run, k], k)


def test_rows_outside_the_filter_give_no_candidate_and_no_mask_is_needed():
    from torchpq_amd.kernels import IVFPQFilteredTopkHip
    case = cases.plain_case(16, 4, "fused", 3, 8, "euclidean")
    g = _gpu(case)
    rows = np.array([-1, len(cases.ROWS), 4], np.int32)
    for n_split in (1, 5):
        v, a, i = IVFPQFilteredTopkHip(m=16)(g["storage"], g["cs"], g["sz"], g["npl"], 10, g["bits"], T(rows),
                                             query=g["query"], codebook=g["codebook"], is_empty=g["is_empty"],
                                             address2id=g["a2i"], n_split=n_split)
        assert torch.all(a[:2] == -1) and torch.all(i[:2] == -1) and torch.all(torch.isneginf(v[:2]))
    # without is_empty the tombstones and free slots inside the probed cells count where their bits are set: the
    # oracle with no tombstone mask
    want = forc.scan_filtered(case["storage"], case["lut"], None, case["allowed"], case["runs"][0], case["cs"],
                              case["sz"], case["npl"], 100)
    v, a = IVFPQFilteredTopkHip(m=16)(g["storage"], g["cs"], g["sz"], g["npl"], 100, g["bits"], g["runs"][0],
                                      precomputed=g["lut"])
    assert np.array_equal(N(a), want[1]) and np.array_equal(N(v).view(np.uint32), want[0].view(np.uint32))


def test_cross_check_with_the_unfiltered_exact_scan():
    """the all-ones row on a layout whose cells stay inside the storage: what IVFPQTopkHip.topk gives on the reference
    layout (tpq_ivfpq_scan_topk / tpq_ivfpq_scan_topk_residual) for the same inputs"""
    from torchpq_amd.kernels import IVFPQTopkHip
    plain = cases.plain_case(16, 4, "fused", 7, 8, "euclidean", over=False)
    res = cases.residual_case(8, 4, "part1", 7, 8, over=False)
    gp, gr = _gpu(plain), _gpu(res)
    last = len(plain["runs"]) - 1                      # the run without filter_of_query: row 0, all ones
    ones = torch.zeros(7, device=DEV, dtype=torch.int32)
    gp["runs"].append(ones)
    gr["runs"].append(ones)
    for k in (1, 10, 100, 1000):
        tv, ta, ti = IVFPQTopkHip(m=16).topk(gp["storage"], gp["lut"], gp["is_empty"], gp["cs"], gp["sz"], gp["npl"],
                                             n_candidates=k, address2id=gp["a2i"])
        for run in (last, last + 1):
            for n_split in (None, 3):
                v, a, i = _run_plain(plain, "fused", "euclidean", run, k, n_split)
                assert torch.equal(a, ta) and torch.equal(i, ti) and torch.equal(v.view(torch.int32), tv.view(torch.int32))
        tv, ta, ti = IVFPQTopkHip(m=8).topk_residual_precomputed(
            gr["storage"], gr["part1"], gr["part2"], gr["cells"], gr["base_sims"], gr["is_empty"], gr["cs"], gr["sz"],
            gr["npl"], n_candidates=k, address2id=gr["a2i"])
        for run in (last, last + 1):
            for tables in ("part1", "built"):
                v, a, i = _run_residual(res, tables, run, k)
                assert torch.equal(a, ta) and torch.equal(i, ti) and torch.equal(v.view(torch.int32), tv.view(torch.int32))
    gp["runs"].pop()
    gr["runs"].pop()


@pytest.mark.parametrize("n_slots,n", [(1, 1), (77, 40), (4096, 1), (100003, 250000)])
def test_slot_filter_build_against_a_bit_pack(n_slots, n):
    """every address in [0, n_slots) sets its bit, repeated ones once; -1, n_slots and beyond are ignored; the words
    behind ceil(n_slots / 32) and the bits already set stay"""
    from torchpq_amd.kernels import SlotFilterBuildHip
    rng = np.random.default_rng(n_slots)
    adr = rng.integers(0, n_slots, n).astype(np.int64)
    adr = np.concatenate([adr, [-1, n_slots, n_slots + 31, -(1 << 40), 1 << 40, n_slots - 1]]).astype(np.int64)
    stride = (n_slots + 31) // 32 + 3
    bits = torch.zeros(stride, device=DEV, dtype=torch.int32)
    out = SlotFilterBuildHip()(T(adr), bits, n_slots)
    assert out is bits
    want = forc.build_bits(adr, n_slots, stride)
    assert np.array_equal(N(bits).view(np.uint32), want) and want.any()
    SlotFilterBuildHip()(T(np.array([0, 5], np.int64)), bits, n_slots)                     # a second set: the union
    want2 = forc.build_bits(np.concatenate([adr, [0, 5]]), n_slots, stride)
    assert np.array_equal(N(bits).view(np.uint32), want2)
    SlotFilterBuildHip()(torch.zeros(0, device=DEV, dtype=torch.int64), bits, n_slots)     # nothing to add
    assert np.array_equal(N(bits).view(np.uint32), want2)


# ---- the index -----------------------------------------------------------------------------------------
def _build(distance, residual, precomputed=True, m=8, seed=0, nq=24, d=32, n_cells=16, n=4000):
    """train, add in two batches with explicit ids, remove some ids"""
    from torchpq_amd.index import IVFPQIndex
    base, queries = _clustered(seed, d, n, nq)
    np.random.seed(seed)
    torch.manual_seed(seed)
    idx = IVFPQIndex(d, n_subvectors=m, n_cells=n_cells, initial_size=16, distance=distance, device=DEV,
                     pq_use_residual=residual)
    idx.train(T(base))
    if residual and not precomputed:
        idx.use_precomputed = False
    ids = torch.arange(n, device=DEV) * 2 + 5
    assert torch.equal(idx.add(T(base[:, :n // 2]), ids=ids[:n // 2]), ids[:n // 2])
    assert torch.equal(idx.add(T(base[:, n // 2:]), ids=ids[n // 2:]), ids[n // 2:])
    removed = np.arange(7, n, 11)
    idx.remove(ids=ids[T(removed)])
    return idx, base, queries, N(ids), removed


def _expected(idx, queries, id_sets, rows, k):
    """tests/ivfpq_filtered_oracle.search_filtered on the index's own state and the cells its coarse step returns; the
    tables are the ones the index would hand its kernels, restated on the CPU where the arithmetic is pinned"""
    x = np.asarray(queries, np.float32)
    if idx.distance == "cosine":
        from torchpq_amd import util
        x = N(util.normalize(T(x), dim=0))
    sims, cells, npl = idx.probe(T(x))
    codebook = N(idx.pq_codec.codebook)
    lut = residual = None
    if not idx.pq_use_residual:
        lut = c_oracle.adc_lut(x, codebook, idx.distance)
    elif idx.use_precomputed:
        if idx._part2_by_cell is None:
            idx.precompute_part2()
        residual = dict(base_sims=N(sims), part1=orc.residual_part1(x, codebook), part2=N(idx._part2_by_cell))
    else:
        residual = dict(base_sims=N(sims), full=N(idx.precomputed_adc_residual(T(x), cells)))
    return forc.search_filtered(N(idx._storage), N(idx._is_empty), N(idx._cell_start), N(idx._cell_size),
                                N(idx._address2id), N(cells), N(npl), id_sets, rows, k, lut=lut, residual=residual)


def _check(idx, queries, flt, id_sets, rows, k):
    v, i = idx.search_filtered(T(queries), k, flt, None if rows is None else T(rows))
    ev, ei, ea = _expected(idx, queries, id_sets, rows, k)
    assert v.dtype == torch.float32 and i.dtype == torch.int64 and v.shape == i.shape == (queries.shape[1], k)
    assert np.array_equal(N(i), ei)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    return N(v), N(i)


@pytest.mark.parametrize("distance,residual,precomputed", [
    ("euclidean", False, True), ("cosine", False, True), ("euclidean", True, True), ("euclidean", True, False)])
def test_index_search_filtered(distance, residual, precomputed):
    idx, base, queries, ids, removed = _build(distance, residual, precomputed, seed=2)
    nq = queries.shape[1]
    rng = np.random.default_rng(5)
    idx.n_probe = 6
    # one shared set: a tenth of the ids, removed ones and ids the index never held among them
    tenth = np.concatenate([rng.choice(ids, len(ids) // 10, replace=False), [-3, 4, 10 ** 9]]).astype(np.int64)
    flt = idx.id_filter(T(tenth))
    v, i = _check(idx, queries, flt, [tenth], None, 10)
    found = i[i >= 0]
    assert len(found) and np.isin(found, tenth).all() and not np.isin(found, ids[removed]).any()
    plain_v, plain_i = idx.search(T(queries), k=10)
    assert not np.array_equal(N(plain_i), i)                               # the filter does change the answer
    _check(idx, queries, flt, [tenth], None, 300)                          # more than most queries can fill
    # per-query rows: everything, one id, nothing, a half
    half = ids[rng.random(len(ids)) < 0.5]
    sets = [ids, ids[1234:1235], np.zeros(0, np.int64), half]
    multi = idx.id_filter([T(s) for s in sets])
    rows = (np.arange(nq) % 4).astype(np.int32)
    v, i = _check(idx, queries, multi, sets, rows, 20)
    assert np.array_equal(i[rows == 0], N(idx.search(T(queries), k=20)[1])[rows == 0])    # every id allowed: search
    assert np.all(i[rows == 2] == -1) and np.all(np.isneginf(v[rows == 2]))           # an empty id set: all padding
    assert np.all(i[rows == 1][:, 1:] == -1) and set(i[rows == 1][:, 0]) <= {-1, int(ids[1234])}
    v64, i64 = idx.search_filtered(T(queries), 20, multi, T(rows.astype(np.int64)))   # any int tensor chooses the rows
    assert np.array_equal(N(i64), i)
    empty = idx.id_filter(torch.zeros(0, dtype=torch.int64))
    v, i = _check(idx, queries, empty, [np.zeros(0, np.int64)], None, 5)
    assert np.all(i == -1) and np.all(np.isneginf(v))
    # a filter made before an add that grows the container gives what one made after gives
    cap_before = idx.capacity
    extra = (base[:, :1500] + 0.01).astype(np.float32)
    new_ids = torch.arange(1500, device=DEV) + 100000
    early = [np.concatenate([half, N(new_ids[::3])]), ids[::7]]
    before = idx.id_filter([T(s) for s in early])
    before.bits()                                                          # built for the old addresses
    idx.add(T(extra), ids=new_ids)
    assert idx.capacity > cap_before
    rows2 = (np.arange(nq) % 2).astype(np.int32)
    got_before = _check(idx, queries, before, early, rows2, 50)
    got_after = _check(idx, queries, idx.id_filter([T(s) for s in early]), early, rows2, 50)
    assert np.array_equal(got_before[1], got_after[1]) and np.isin(got_before[1], N(new_ids)).any()
    assert np.array_equal(got_before[0].view(np.uint32), got_after[0].view(np.uint32))
    # ... and follows a remove
    gone = got_before[1][0][got_before[1][0] >= 0][:5]
    idx.remove(ids=T(gone))
    after_remove = _check(idx, queries, before, early, rows2, 50)
    assert not np.isin(after_remove[1], gone).any()
    # a batch larger than max_query_batch equals the unbatched call: the rows are cut alongside the queries
    idx.max_query_batch = 7
    batched = _check(idx, queries, before, early, rows2, 50)
    idx.max_query_batch = 32768
    assert np.array_equal(batched[1], after_remove[1])
    assert np.array_equal(batched[0].view(np.uint32), after_remove[0].view(np.uint32))
    # search_cells_filtered hands back the addresses too
    x = idx._prepare(T(queries))
    sims, cells, npl = idx.probe(x)
    cv, ci, ca = idx.search_cells_filtered(x, cells, before, T(rows2), base_sims=sims, n_probe_list=npl, k=50,
                                           return_address=True)
    assert np.array_equal(N(ci), after_remove[1]) and torch.equal(idx.get_id_by_address(ca)[ca >= 0], ci[ca >= 0])
    none = idx.search_filtered(T(queries[:, :0]), 5, before)
    assert none[0].shape == none[1].shape == (0, 5)


def test_long_subvectors_take_the_materialised_table_and_no_scan_layout_copy_is_built():
    for residual in (False, True):
        idx, base, queries, ids, removed = _build("euclidean", residual, m=4, seed=4)
        assert idx.d_subvector > idx.fused_lut_max_subvector
        idx.n_probe = 5
        sets = [ids[::3], ids[::50]]
        rows = (np.arange(queries.shape[1]) % 2).astype(np.int32)
        _check(idx, queries, idx.id_filter([T(s) for s in sets]), sets, rows, 10)
        assert idx._packed is None                                         # the filtered route reads _scan_codes()


def test_ivfpqr_index_raises():
    from torchpq_amd.index import IVFPQRIndex
    idx = IVFPQRIndex(32, n_subvectors=8, n_subvectors_rerank=8, n_cells=16, device=DEV)
    with pytest.raises(NotImplementedError):
        idx.search_filtered(torch.zeros(32, 2, device=DEV), 5, None)
