"""GPU: scan_finish_exact_kernel (csrc/scan_finish.h) at the shapes where its deal of the queries, the seeds it no
longer evaluates and the chunks it no longer reads can go wrong.  Every result is compared with oracle/c_oracle
(adc_lut + scan_topk on the same probes): values bit for bit, addresses entry by entry.

  the deal   workgroup b of G takes the queries [b nq / G, (b + 1) nq / G) and its waves draw them from a counter in LDS:
             batches of 1 024 ... 4 097 queries on the cell-major form (whose stage 1 ends with a split tail from 1 025
             on); the query-major route at m = 32 and the table-gathering form (FROM_LUT, two workgroups per CU) at batches
             around 16 queries per workgroup and just past 16 x the CU count; a query-major batch with a split tail.
             The product library takes the large-batch routes, the only ones that end with this kernel, from 1 024
             queries on (kDumpMinQueries): batches of 1, 15, 16 and 17 queries run other kernels (their ids say so) and are
             compared all the same; 1 024 + {15, 16, 17} queries are the smallest batches that give a workgroup of the finish kernel a
             range of 15, 16 and 17 queries (65 and 66 workgroups).
  the seeds  k = 1 ... 128 (one and two seed chunks, full and partly pad); no candidate at all; every seed below the
             cut; fewer than k seeds (tau = -inf, pad seeds); one vector stored in a seed cell and in a later cell;
             tombstones in the seed cells.
  the fill   exactly 0, 1, 63, 64, 65, capacity and capacity + 1 entries behind the seed chunks, in the 16-chunk form
             (k = 100: capacity 14 x 64) and in the 8-chunk form (k = 10: the workspace of a small k; capacity 7 x 64) --
             the counts are exact because the seed cells hold fewer than k live slots, so tau = -inf and every live slot
             of the later probes is appended; capacity + 1 flags the query, and only that one; a workspace that held long
             lists used again for short ones; flagged queries (a NaN component, an all-zero query) inside a workgroup's
             range."""
import functools

import numpy as np
import pytest
import torch

from oracle import c_oracle
from test_gpu_scan_cells import DEV, P0, _problem, _search

pytestmark = pytest.mark.gpu

THREADS = 8
FAR = 224          # the code bytes from here on decode to entries far from every query (_far_codebook)


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def _np(t):
    return None if t is None else t.cpu().numpy()


def _extents(p):
    cells = p["cells"].clamp(0, p["n_cells"] - 1)
    return p["start"][cells].contiguous(), (p["sz"] if "sz" in p else p["sizes"][cells]).contiguous()


def _oracle(p, k, distance="euclidean", lut=None):
    """(values, addresses) of c_oracle.scan_topk, the table built by c_oracle.adc_lut 512 queries at a time"""
    cs, sz = (_np(t) for t in _extents(p))
    storage, emp, npl = _np(p["storage"]), _np(p["is_empty"]), _np(p["npl"])
    query, codebook = _np(p["query"]), _np(p["codebook"])
    nq = query.shape[1]
    vals, addr = np.empty((nq, k), np.float32), np.empty((nq, k), np.int64)
    for b in range(0, nq, 512):
        e = min(nq, b + 512)
        t = c_oracle.adc_lut(query[:, b:e], codebook, distance, n_threads=THREADS) if lut is None else lut[:, b:e]
        vals[b:e], addr[b:e] = c_oracle.scan_topk(storage, t, emp, cs[b:e], sz[b:e], npl[b:e], k, n_threads=THREADS)
    return vals, addr


def _same(got, want, k=None, skip=()):
    """bit-equal values and equal addresses; `k`: the oracle ran with a larger k (a top-k under a strict total order is a
    prefix of every longer one); `skip`: rows whose values are NaN"""
    v, a = _np(got[0]), _np(got[1])
    wv, wa = (want[0], want[1]) if k is None else (want[0][:, :k], want[1][:, :k])
    rows = np.setdiff1d(np.arange(v.shape[0]), np.asarray(skip, np.int64))
    assert np.array_equal(np.ascontiguousarray(v[rows]).view(np.int32), np.ascontiguousarray(wv[rows]).view(np.int32))
    assert np.array_equal(a[rows], wa[rows])


def _form(p, k, distance="euclidean", scan=None):
    got, scan = _search(p, k, distance, scan=scan)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is True
    return got, scan


def _first(p, nq):
    """the first nq queries of a problem (the storage and its scan-layout copy are shared)"""
    q = dict(p)
    q["query"], q["cells"], q["npl"] = p["query"][:, :nq].contiguous(), p["cells"][:nq].contiguous(), p["npl"][:nq].contiguous()
    if "sz" in p:
        q["sz"] = p["sz"][:nq].contiguous()
    return q


# ---- the deal: the cell-major form ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _big():
    """4 097 queries over 16 cells of 0 ... 300 slots, 8 ragged probes, tombstones; the oracle's top-100 of all of them"""
    p = _problem(4097, 4097, 16, 8, 2)
    return p, _oracle(p, 100)


@pytest.mark.parametrize("nq", [1024, 1025, 4095, 4096, 4097])
def test_deal_on_the_cell_major_form(nq):
    """on 256 CUs: 64 and 65 workgroups with ranges of 15 and 16 queries; 256 workgroups with ranges of 15 and 16, of 16,
    of 16 and 17.  From 1 025 queries on the threshold pass deals its last queries in parts (rank / unsplit)"""
    p, want = _big()
    got, scan = _form(_first(p, nq), 100)
    _same(got, (want[0][:nq], want[1][:nq]))
    assert scan.last_redone(nq) < nq // 10


# ---- the deal: query-major routes at m = 32 ---------------------------------------------------------------------------------
def _problem_m32(seed, nq, ds=4, n_cells=16, n_probe=8):
    rng = np.random.default_rng(seed)
    m = 32
    sizes = np.array(([0, 1, 63, 64, 65, 255, 257, 300] * 2)[:n_cells])
    cap = sizes + 3
    start = np.cumsum(cap) - cap
    n_slots = int(cap.sum())
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    npl = rng.integers(0, n_probe + 1, nq)
    npl[:3] = [n_probe, 0, 1][:min(nq, 3)]
    return dict(storage=T(rng.integers(0, 256, (m // 4, n_slots, 4), dtype=np.uint8)),
                codebook=T((rng.standard_normal((m, ds, 256)) * 3).astype(np.float32)),
                query=T((rng.standard_normal((m * ds, nq)) * 3).astype(np.float32)),
                is_empty=T((rng.random(n_slots) < 0.05).astype(np.uint8)), cells=T(cells), npl=T(npl.astype(np.int64)),
                start=T(start), sizes=T(sizes), n_cells=n_cells, n_slots=n_slots)


def _n_past_the_grid(per_cu):
    """one query more than 16 for every workgroup of a full grid"""
    return 16 * per_cu * torch.cuda.get_device_properties(DEV).multi_processor_count + 1


@functools.lru_cache(maxsize=None)
def _m32(from_lut):
    from torchpq_amd import kernels as K
    nq = _n_past_the_grid(2 if from_lut else 1)
    p = _problem_m32(32 + from_lut, nq)
    p["packed"] = K.PackCodesHip()(p["storage"])
    lut = c_oracle.adc_lut(_np(p["query"]), _np(p["codebook"]), n_threads=THREADS) if from_lut else None
    return p, lut, _oracle(p, 10, lut=lut)


def _search_m32(p, k, lut=None):
    from torchpq_amd import kernels as K
    scan = K.IVFPQTopkHip(m=32)
    cs, sz = _extents(p)
    if lut is None:
        out = scan.topk_fused(p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], k,
                              packed=p["packed"], n_split=1, slots_hint=1000)
    else:   # (the table-gathering form pays behind long scans only: the hint says so, the lists stay short)
        out = scan.topk(p["storage"], torch.from_numpy(np.ascontiguousarray(lut)).to(DEV), p["is_empty"], cs, sz,
                        p["npl"], n_candidates=k, packed=p["packed"], n_split=1, slots_hint=30000)
    torch.cuda.synchronize()
    return out, scan


@pytest.mark.parametrize("from_lut", [False, True], ids=["codebook", "from_lut"])
@pytest.mark.parametrize("nq", [pytest.param(n, id="%d-another_route" % n) for n in (1, 15, 16, 17)] +
                         [1024, 1039, 1040, 1041, "past the grid"])
def test_deal_on_the_query_major_routes_at_m32(nq, from_lut):
    """the finish kernel runs from 1 024 queries on (asserted through the route); the smaller batches the issue names run
    another route's kernels, as their ids say, and only pin the results"""
    p, lut, want = _m32(from_lut)
    nq = p["query"].shape[1] if nq == "past the grid" else nq
    got, scan = _search_m32(_first(p, nq), 10, None if lut is None else lut[:, :nq])
    assert (scan.last_route() == "dump_f32") is (nq >= 1024)
    _same(got, (want[0][:nq], want[1][:nq]))


def _tail_parts(scan, nq):
    """Parts the last call dealt its split tail in, from the library's own plan (tpq_ivfpq_scan_ordered: host arithmetic
    for the device the call ran on).  The plan orders a batch of more than one round exactly when the workspace holds
    the lists in use -- flags, bands, parts x 4 waves x RL chunks of 512 bytes, eviction words -- and three int32 per
    query behind them; one byte less and it does not.  A plan that kept the tail whole would already order the call with
    the room its four lists leave.  Lists of 16 chunks per query: 4 parts of one-register lists or 2 of two-register ones"""
    al = lambda n: (n + 255) // 256 * 256  # noqa: E731
    for parts, rl in ((4, 1), (2, 2)):
        lists = 2 * al(4 * nq) + nq * 4 * parts * rl * 512 + al(4 * nq * 4 * parts)
        need = lists + 3 * al(4 * nq)
        if scan.last_workspace_bytes >= lists and scan.ordered(need) and not scan.ordered(need - 1):
            return parts
    return 1


@pytest.mark.parametrize("k,parts", [(10, 4), (100, 2)])
def test_split_tail_inside_a_workgroups_range(k, parts):
    """query-major at m = 64, five quarters of the workgroup slots the device gives the scan kernel: the last fifth of
    the queries, longest first, is dealt in 4 (k = 10) or 2 (k = 100) parts -- asserted on the library's plan --, so the
    queries of one workgroup's range come with 4 and with 16 chunks (8 and 16), by their rank in the dispatch order"""
    p, want = _big()
    slots = 4 * torch.cuda.get_device_properties(DEV).multi_processor_count
    nq = slots + slots // 4
    assert 1024 <= nq <= 4097
    q = _first(p, nq)
    got, scan = _search(q, k, cells=False)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is False
    assert _tail_parts(scan, nq) == parts          # n_split > 1; unsplit = the `slots` queries of the first round > 0
    _same(got, (want[0][:nq], want[1][:nq]), k=k)


# ---- the seeds -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _seeded():
    p = _problem(128, 1024, 16, 8, 2)
    return p, _oracle(p, 128)


@pytest.mark.parametrize("k", [1, 63, 64, 65, 100, 128])
def test_seed_chunks_of_every_length(k):
    """one seed chunk partly filled, full, two chunks with 1, 36 and 64 seeds in the second"""
    p, want = _seeded()
    got, scan = _form(p, k)
    _same(got, want, k=k)
    assert scan.last_redone(1024) < 1024 // 10


def _far_codebook(rng, ds):
    """entries 0 ... 223 as everywhere (N(0, 3^2) like the queries), entries 224 ... 255 of every sub-quantizer shifted
    by 10 in every component: at ds = 2 a slot of FAR codes has a value of -15 000 +- 1 000 under every query, the others
    -2 300 +- 300, and 2 delta stays near 5 (a larger shift would widen the band with |x|max^2)"""
    cb = (rng.standard_normal((64, ds, 256)) * 3).astype(np.float32)
    cb[:, :, FAR:] += 10.0
    return cb


def _near_far(seed, far_first, nq=1024, ds=2):
    """8 cells, every query probes all of them: four `near` cells (codes 0 ... 223) and four `far` cells (codes 224 ...
    255), the far ones first or last"""
    rng = np.random.default_rng(seed)
    sizes = np.array([60, 70, 65, 64, 100, 90, 110, 120])
    cap = sizes + 2
    start = np.cumsum(cap) - cap
    n_slots = int(cap.sum())
    storage = rng.integers(0, FAR, (16, n_slots, 4), dtype=np.uint8)
    far_cells, near_cells = ([0, 1, 2, 3], [4, 5, 6, 7]) if far_first else ([4, 5, 6, 7], [0, 1, 2, 3])
    for c in far_cells:
        storage[:, start[c]:start[c] + sizes[c], :] = rng.integers(FAR, 256, (16, sizes[c], 4), dtype=np.uint8)
    first, later = (far_cells, near_cells) if far_first else (near_cells, far_cells)
    rows = np.stack([np.concatenate([rng.permutation(first), rng.permutation(later)]) for _ in range(nq)])
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(storage=T(storage), codebook=T(_far_codebook(rng, ds)),
                query=T((rng.standard_normal((64 * ds, nq)) * 3).astype(np.float32)),
                is_empty=T((rng.random(n_slots) < 0.05).astype(np.uint8)), cells=T(rows),
                npl=T(np.full(nq, 8, np.int64)), start=T(start), sizes=T(sizes), n_cells=8, n_slots=n_slots,
                hint=int(sizes.sum()))


def _appended(p, tau):
    """entries the candidate kernel appends for the probes from P0 on under the thresholds tau"""
    from torchpq_amd import kernels as K
    cs, sz = _extents(p)
    count, _, _, _, flags = K.CellCandidatesHip()(p["storage"], p["query"], p["codebook"], p["cells"], p["n_cells"], cs, sz,
                                                  p["npl"], torch.from_numpy(np.ascontiguousarray(tau)).to(DEV),
                                                  first_probe=P0, capacity=1024, is_empty=p["is_empty"])
    assert not flags.any().item()
    return _np(count)


def test_top_k_wholly_in_the_first_probes():
    """the later probes hold far slots only: nothing is appended (asserted on the candidate kernel under the same
    thresholds), stage 5 sees the seed chunks alone and writes them back"""
    k = 100
    p = _near_far(200, far_first=False)
    want = _oracle(p, k)
    assert np.isfinite(want[0]).all()
    assert (_appended(p, want[0][:, k - 1]) == 0).all()
    got, scan = _form(p, k)
    _same(got, want)
    assert scan.last_redone(1024) == 0


def test_every_seed_below_the_cut():
    """the caller's cell order puts the far cells first: the seeds are far slots, tau admits every live slot of the later
    probes, and the cut F_k - 2 delta of stage 5 lies above every seed"""
    k = 100
    p = _near_far(201, far_first=True)
    want = _oracle(p, k)
    start, sizes, emp = _np(p["start"]), _np(p["sizes"]), _np(p["is_empty"])
    assert ((want[1] >= start[4]) & (want[1] < start[7] + sizes[7])).all()     # no seed is part of any result
    seeds = dict(p, npl=torch.full_like(p["npl"], P0))
    tau = _oracle(seeds, k)[0][:, k - 1]                                         # the k-th seed: a far slot
    assert np.isfinite(tau).all() and (tau < want[0][:, k - 1] - 5000).all()
    live = sum(int((emp[start[c]:start[c] + sizes[c]] == 0).sum()) for c in (4, 5, 6, 7))
    assert (_appended(p, tau) == live).all()
    got, scan = _form(p, k)
    _same(got, want)
    assert scan.last_redone(1024) == 0


def test_fewer_than_k_seeds():
    """the first four cells hold 17 slots: tau = -inf, the seed chunks are mostly pad, everything else is appended"""
    p = _problem(12, 1024, 8, 8, 2, sizes=[3, 5, 2, 7, 1, 120, 130, 140], ragged=False)
    p["cells"] = torch.arange(8, device=DEV).repeat(1024, 1).contiguous()
    for k in (100, 128):
        got, scan = _form(p, k)
        _same(got, _oracle(p, k))
        assert scan.last_redone(1024) == 0


def test_one_vector_in_a_seed_cell_and_in_a_later_cell():
    """the codes of 60 slots of the first cell stored again in the sixth: equal values in a seed chunk and among the
    candidates, the smaller address first"""
    k = 100
    p = _problem(203, 1024, 8, 8, 2, sizes=[64, 65, 63, 70, 100, 90, 110, 120], ragged=False, holes=False)
    p["cells"] = torch.arange(8, device=DEV).repeat(1024, 1).contiguous()
    s0, s5 = int(p["start"][0]), int(p["start"][5])
    p["storage"][:, s5:s5 + 60, :] = p["storage"][:, s0:s0 + 60, :]
    want = _oracle(p, k)
    twice = sum(int(np.isin(want[1][q], np.arange(s5, s5 + 60)).sum()) for q in range(1024))
    assert twice > 1024                                                   # (the pairs do reach the results)
    got, _ = _form(p, k)
    _same(got, want)


def test_tombstones_in_the_seed_cells():
    k = 100
    p = _problem(204, 1024, 8, 8, 2, sizes=[120, 130, 110, 140, 100, 90, 110, 120], ragged=False)
    p["cells"] = torch.arange(8, device=DEV).repeat(1024, 1).contiguous()
    g = torch.Generator(device=DEV)
    g.manual_seed(205)
    seed_slots = int(p["start"][4])
    p["is_empty"][:seed_slots] = (torch.rand(seed_slots, generator=g, device=DEV) < 0.4).to(torch.uint8)
    got, _ = _form(p, k)
    _same(got, _oracle(p, k))


# ---- the fill ---------------------------------------------------------------------------------------------------------------------
def _filled(seed, k, counts, nq=1024, nan=(), zero=()):
    """Four seed cells with k // 2 live slots between them (tau = -inf), a cell of exactly n live slots for every n of
    `counts`, one void cell.  Query q probes the seed cells, then the cell of counts[q % len(counts)], then the void
    cell: cnt[q] is exactly that n."""
    rng = np.random.default_rng(seed)
    seeds = [k // 2 - 3 * (k // 8), k // 8, k // 8, k // 8]
    sizes = np.array(seeds + list(counts) + [0])
    cap = sizes + 1
    start = np.cumsum(cap) - cap
    n_slots = int(cap.sum())
    rows = np.array([[0, 1, 2, 3, 4 + q % len(counts), 4 + len(counts)] for q in range(nq)])
    query = (rng.standard_normal((128, nq)) * 3).astype(np.float32)
    for q in nan:
        query[5, q] = np.nan
    for q in zero:
        query[:, q] = 0.0
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return dict(storage=T(rng.integers(0, 256, (16, n_slots, 4), dtype=np.uint8)),
                codebook=T((rng.standard_normal((64, 2, 256)) * 3).astype(np.float32)), query=T(query), is_empty=None,
                cells=T(rows), npl=T(np.full(nq, 6, np.int64)), start=T(start), sizes=T(sizes), n_cells=len(sizes),
                n_slots=n_slots, hint=int(sum(seeds) + np.mean(counts)))


@pytest.mark.parametrize("k,chunks", [(100, 16), (10, 8)])
def test_lists_filled_to_every_length(k, chunks):
    """0, 1, 63, 64, 65 entries behind the seed chunks, the capacity and one more.  That exactly the queries of the last
    count are redone also says which form ran: 14 x 64 + 1 entries fit the other form's lists at k = 10, and 7 x 64 + 1
    overflow only the 8-chunk form"""
    cap = (chunks - (k + 63) // 64) * 64
    counts = [0, 1, 63, 64, 65, cap, cap + 1]
    p = _filled(300 + k, k, counts)
    got, scan = _form(p, k)
    _same(got, _oracle(p, k))
    assert scan.last_redone(1024) == len(range(6, 1024, 7))


def test_dirty_workspace_long_lists_then_short_ones():
    """one scan object, the same block of memory (asserted): a batch that fills its lists to the capacity, then a batch
    of the same shape with at most 65 entries behind the seeds -- the chunks behind them still hold the first batch's keys"""
    from torchpq_amd import kernels as K
    k = 100
    long_, short = _filled(310, k, [896, 890, 800, 896, 700]), _filled(311, k, [0, 1, 63, 64, 65])
    want_long, want_short = _oracle(long_, k), _oracle(short, k)
    short["packed"] = K.PackCodesHip()(short["storage"])    # (nothing is allocated between the two calls but the workspace)
    scan = K.IVFPQTopkHip(m=64)
    got, scan = _form(long_, k, scan=scan)
    _same(got, want_long)
    block, size = scan.last_workspace.data_ptr(), scan.last_workspace_bytes
    scan.last_workspace = None     # (the allocator hands the next call of this size the same block)
    got, scan = _form(short, k, scan=scan)
    assert scan.last_workspace.data_ptr() == block and scan.last_workspace_bytes == size
    _same(got, want_short)
    assert scan.last_redone(1024) == 0


def test_flagged_queries_inside_a_workgroups_range():
    """1 024 queries are 64 ranges of 16: queries 8 and 1 000 carry a NaN, 9 and 520 are all zero (the form cannot scale
    them) -- all four are left to the exact kernel, their neighbours are not"""
    k = 100
    p = _filled(320, k, [0, 1, 63, 64, 65, 200, 896], nan=(8, 1000), zero=(9, 520))
    got, scan = _form(p, k)
    _same(got, _oracle(p, k), skip=(8, 1000))
    assert scan.last_redone(1024) == 4
