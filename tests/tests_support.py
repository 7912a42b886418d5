"""Helpers shared between test modules: the k-means fit cases, and the IVFPQRIndex re-rank cases and checks."""
import numpy as np
import torch

# shared by the k-means fit tests: name -> (init key, n_redo, max_iter, tol key or value, seed key)
CASES = {
    "1": ("init", 1, 1, 0.0, None),
    "3": ("init", 1, 3, 0.0, None),
    "tol": ("init", 1, 12, "tol_exit", None),
    "redo": ("init", 2, 3, 0.0, "redo_seed"),
    "redo_b": ("bad_init", 2, 3, 0.0, "redo_b_seed"),
}

# ---- shared by the IVFPQRIndex GPU tests (test_gpu_ivfpqr.py, test_gpu_ivfpqr_edges.py) ----------------
DEV = "cuda:0"


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def N(t):
    return t.detach().cpu().numpy()


def _case(seed, m, m_r, d, cap, nq, k1, distance, scale=None):
    """a random re-rank problem; `scale` (codebooks and query, for long vectors) multiplies after generation, so
    a case without it is what it always was"""
    rng = np.random.default_rng(seed)
    storage = rng.integers(0, 256, ((m + m_r) // 4, cap, 4), dtype=np.uint8)
    cb = rng.standard_normal((m, d // m, 256)).astype(np.float32)
    cb_r = (0.3 * rng.standard_normal((m_r, d // m_r, 256))).astype(np.float32)
    query = rng.standard_normal((d, nq)).astype(np.float32)
    if distance == "cosine":
        query = (query / np.linalg.norm(query, axis=0, keepdims=True)).astype(np.float32)
    cand = np.argsort(rng.random((nq, cap)), axis=1)[:, :k1].astype(np.int64)   # distinct per row
    # rows with fewer than k real candidates (holes anywhere in the row), and rows with none
    short = rng.random(nq) < 0.3
    cand[short[:, None] & (rng.random((nq, k1)) < 0.7)] = -1
    cand[rng.random(nq) < 0.1] = -1
    if nq >= 3:
        cand[1] = -1
    a2i = rng.permutation(cap).astype(np.int64) * 3 + 1
    if scale is not None:
        cb, cb_r = (cb * np.float32(scale)).astype(np.float32), (cb_r * np.float32(scale)).astype(np.float32)
        if distance != "cosine":
            query = (query * np.float32(scale)).astype(np.float32)
    return storage, cb, cb_r, query, cand, a2i


def _run_and_compare(storage, cb, cb_r, query, cand, a2i, k, use_residual, distance, m):
    import ivfpqr_oracle as rorc
    from torchpq_amd.kernels import IVFPQRerankHip
    v, a, i = IVFPQRerankHip()(T(storage), m, T(cb) if use_residual else None, T(cb_r), T(query), T(cand), k,
                               use_residual=use_residual, distance=distance, address2id=T(a2i))
    ev, ea, ei = rorc.rerank(storage, cb, cb_r, query, cand, k, use_residual, distance, a2i)
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(N(i), ei)
    return N(v), N(a), N(i)


def _clustered(seed, d, n, nq, n_centers=40, spread=4.0):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((d, n_centers)) * spread
    base = (centers[:, rng.integers(0, n_centers, n)] + rng.standard_normal((d, n))).astype(np.float32)
    queries = (base[:, rng.choice(n, nq, replace=False)] + 0.3 * rng.standard_normal((d, nq))).astype(np.float32)
    return base, queries


def _normalize(idx, x):
    from torchpq_amd import util
    return util.normalize(x, dim=0)


def _expected_search(idx, x, k, rows=None):
    """tests/ivfpqr_oracle.search driven by the index's own coarse step (the pattern of test_gpu_index.py);
    `rows`: only these queries of the batch (the coarse step still sees the whole batch)"""
    import ivfpqr_oracle as rorc
    x = np.asarray(x, dtype=np.float32)
    if idx.distance == "cosine":
        x = N(_normalize(idx, T(x)))
    _, cells, npl = idx.probe(T(x))
    cells, npl = N(cells), N(npl)
    if rows is not None:
        x, cells, npl = np.ascontiguousarray(x[:, rows]), np.ascontiguousarray(cells[rows]), npl[rows]
    return rorc.search(x, N(idx.pq_codec.codebook), N(idx.pq_rerank_codec.codebook), N(idx._storage),
                       N(idx._is_empty), N(idx._cell_start), N(idx._cell_size), N(idx._address2id), cells,
                       npl, k, idx.rerank_factor, idx.use_residual, idx.distance)


def _check_search(idx, queries, k):
    v, i, a = idx.search(T(queries), k=k, return_address=True)
    ev, ei, ea = _expected_search(idx, queries, k)
    assert v.shape == (queries.shape[1], k) and v.dtype == torch.float32 and i.dtype == torch.int64
    assert np.array_equal(N(a), ea)
    assert np.array_equal(N(v).view(np.uint32), ev.view(np.uint32))
    assert np.array_equal(N(i), ei)
    v2, i2 = idx.search(T(queries), k=k)
    assert torch.equal(v2, v) and torch.equal(i2, i)
    return N(v), N(i)


# ---- shared by the rounding-band scan tests (test_scan_band_inputs_cpu.py, test_gpu_scan_rounding_band.py) ----
# Inputs on which the fp32 summation ORDER decides the k-th place: look-up tables whose entries share a large offset, so
# that sum_j max|LUT_j| (what the scan's candidate band is proportional to) is far above the spread of the candidates.
BAND_LADDER = (0, 2 ** 10, 2 ** 14, 2 ** 20)
# a table built from a query at distance sqrt(A) of an N(0,1) codebook is -A +- 2 sqrt(A) N(0,1): its spread grows with
# the offset, and the two summation orders only part from about this rung on
FAR_RUNG = 2 ** 30


def offset_lut(rng, m, nq, A, mode):
    """fp32 [m, nq, 256] table.  "far": -A + N(0,1), a euclidean table of a query far from the codebook; "cancel":
    offsets +-A (1 + 0.37 (j // 2)) that cancel in pairs, plus N(0,1) -- the sums stay O(sqrt(m)) while sum_j max|LUT_j|
    grows with A; "mixed": per-sub-quantizer scales from {1e-3, 1, 1e3} times N(0,1), the far offset on a random half
    of the j."""
    A = float(A)
    noise = rng.standard_normal((m, nq, 256))
    j = np.arange(m)
    if mode == "far":
        lut = noise - A
    elif mode == "cancel":
        off = np.where(j % 2 == 0, 1.0, -1.0) * A * (1.0 + 0.37 * (j // 2))
        lut = noise + off[:, None, None]
    elif mode == "mixed":
        scale = rng.choice(np.array([1e-3, 1.0, 1e3]), m)
        lut = noise * scale[:, None, None] - np.where(rng.permutation(m) < m // 2, A, 0.0)[:, None, None]
    else:
        raise ValueError(mode)
    return lut.astype(np.float32)


def offset_query_codebook(rng, m, ds, nq, A, distance):
    """codebook N(0,1) [m, ds, 256] and query N(0,1) + c [m ds, nq] with |LUT| ~ A: euclidean -|q - c|^2 ~ ds c^2,
    inner q . c ~ c sqrt(ds) N(0,1) (for the routes that build the table in the workgroup)"""
    cb = rng.standard_normal((m, ds, 256)).astype(np.float32)
    c = np.sqrt(A / ds) if distance == "euclidean" else A / np.sqrt(ds)
    q = (rng.standard_normal((m * ds, nq)) + c).astype(np.float32)
    return q, cb


def scan_candidates(case, q):
    """slots query q scans, in the reference kernel's sense: its first n_probe_list[q] cells (a cell listed again
    right after itself is skipped), tombstones left out; ascending, each slot once"""
    seen, prev = [], None
    for p in range(int(case["npl"][q])):
        st, sz = int(case["cs"][q, p]), int(case["sz"][q, p])
        if st != prev and sz > 0:
            seen.append(np.arange(st, st + sz))
        prev = st
    slots = np.unique(np.concatenate(seen)) if seen else np.zeros(0, np.int64)
    return slots[case["is_empty"][slots] == 0]


def pairwise_topk_sets(case, lut, k, queries=None):
    """per query, the address set of the top-k (value descending, address ascending) when the m table entries are
    summed PAIRWISE in fp32 (a balanced tree) instead of the reference's ascending-j chain: a stand-in for "another
    summation order", not any kernel's own"""
    g, cap, _ = case["storage"].shape
    codes = case["storage"].transpose(0, 2, 1).reshape(g * 4, cap)        # [m, slot]
    out = []
    for q in (range(lut.shape[1]) if queries is None else queries):
        slots = scan_candidates(case, q)
        t = lut[np.arange(g * 4)[:, None], q, codes[:, slots]].T.astype(np.float32)   # [n, m]
        while t.shape[1] > 1:
            odd = t[:, -1:] if t.shape[1] % 2 else None
            t = (t[:, 0:t.shape[1] - (t.shape[1] % 2):2] + t[:, 1::2]).astype(np.float32)
            if odd is not None:
                t = np.concatenate([t, odd], axis=1)
        order = np.lexsort((slots, -t[:, 0].astype(np.float64)))[:k]
        out.append(set(slots[order].tolist()))
    return out


def orders_disagree(case, lut, k, queries=None):
    """queries (indices) whose top-k address set under the pairwise sum differs from the oracle's"""
    from oracle import c_oracle
    _, ea = c_oracle.scan_topk(case["storage"], lut, case["is_empty"], case["cs"], case["sz"], case["npl"], k)
    qs = list(range(lut.shape[1]) if queries is None else queries)
    pw = pairwise_topk_sets(case, lut, k, qs)
    return [q for q, s in zip(qs, pw) if s != set(ea[q][ea[q] >= 0].tolist())]


def band_index(seed, m, nq, n_probe, tomb=0):
    """the index of test_scan_random_vs_oracle (40 ragged cells of ~150 slots, some empty, optional tombstones) and a
    probe list per query; query 3 lists one cell twice in a row, the first five queries use every probe"""
    from test_gpu_kernels import _random_index
    rng = np.random.default_rng(seed)
    n_cells = 40
    storage, is_empty, start, sizes, a2i = _random_index(rng, m, n_cells, 150, tomb, 0.0)
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    if nq > 3:
        cells[3, 1] = cells[3, 0]
    npl = rng.integers(1, n_probe + 1, nq).astype(np.int64)
    npl[:5] = n_probe
    return dict(storage=storage, is_empty=is_empty, start=start, sizes=sizes, a2i=a2i, cells=cells, npl=npl,
                cs=start[cells], sz=sizes[cells], rng=rng)


def _band_case(route, m, k, A, mode=None, n_split=1, nq=37, n_probe=8, tomb=0, src="lut", ds=0, distance="euclidean",
               hint=None, packed=True, expect=None, disagree=None):
    """one case of the rounding-band tests.  `expect`: the regime seen on the MI355X and asserted since -- "held" (no query
    redone although the CPU check says the two orders pick different members), "redone" (at least one query handed to
    the exact kernel), None (not asserted).  `disagree`: what test_scan_band_inputs_cpu.py asserts about the inputs --
    True (some query's k-set differs between the chain and the pairwise sum), False (none does), None (not asserted)."""
    what = mode if src == "lut" else f"{distance[:3]}{ds}"
    cid = f"{route}-m{m}-k{k}-s{n_split}-{src}-{what}-A{int(np.log2(A)) if A else 0}" + (f"-t{tomb}" if tomb else "") + ("" if packed else "-nopack")
    return dict(id=cid, route=route, m=m, k=k, A=A, mode=mode, n_split=n_split, nq=nq, n_probe=n_probe, tomb=tomb,
                src=src, ds=ds, distance=distance, hint=hint, packed=packed, expect=expect,
                disagree=False if (disagree is None and A == 0) else disagree)


def band_case_inputs(case):
    """index, probe lists and the table of a case (src "lut": offset_lut; "fused": the table c_oracle.adc_lut builds from
    offset_query_codebook, which is what the workgroup builds); seeded by the case's id"""
    import zlib
    from oracle import c_oracle
    ix = band_index(zlib.crc32(case["id"].encode()), case["m"], case["nq"], case["n_probe"], case["tomb"])
    rng = ix["rng"]
    if case["src"] == "lut":
        ix["lut"] = offset_lut(rng, case["m"], case["nq"], case["A"], case["mode"])
    else:
        ix["query"], ix["codebook"] = offset_query_codebook(rng, case["m"], case["ds"], case["nq"], max(case["A"], 1),
                                                            case["distance"])
        ix["lut"] = c_oracle.adc_lut(ix["query"], ix["codebook"], case["distance"])
    return ix


def _band_cases():
    L, modes, out = BAND_LADDER, ("far", "cancel", "mixed"), []
    add = lambda *a, **kw: out.append(_band_case(*a, **kw))
    # the one-launch finish, a caller's table: every chunk layout (m = 12: 4 bytes, 8: 8, 16 ... 128: 16; m = 128: the
    # two-wave reduction of the bound), the ladder with mode, k and the split rotating ...
    for i, m in enumerate((8, 12, 16, 32, 64, 128)):
        for r, A in enumerate(L):
            add("one_launch_finish", m, (1, 10, 100)[(i + r) % 3], A, modes[(i + r) % 3], n_split=(1, 3)[(i + r) % 2],
                tomb=(0, 25)[r % 2])
    # ... and in full at m = 64, k = 100 (the headline shape), m = 8, k = 10
    for m, k in ((64, 100), (8, 10)):
        for mode in modes:
            for A in L:
                add("one_launch_finish", m, k, A, mode, n_split=3 if mode == "cancel" else 1)
    # the table built in the workgroup
    for m, ds in ((8, 4), (16, 2), (64, 2), (128, 1)):
        for distance in ("euclidean", "inner"):
            for r, A in enumerate(L + ((FAR_RUNG,) if distance == "euclidean" else ())):
                add("one_launch_finish", m, (10, 100)[r % 2], A, src="fused", ds=ds, distance=distance,
                    n_split=(1, 3)[r % 2])
    # k > 248: the pools (short codes), the sorted lists of the three-launch path (m = 64 below the pools' k; sixteen waves)
    for m in (8, 16, 32):
        for r, A in enumerate(L):
            add("pools", m, 300, A, modes[r % 3], n_split=(1, 3)[r % 2], n_probe=12)
    for r, A in enumerate(L):
        add("pools", 32, 300, A, src="fused", ds=4, distance=("euclidean", "inner")[r % 2], n_probe=12)
        add("sorted_lists", 64, 300, A, modes[(r + 1) % 3], n_split=(3, 1)[r % 2], n_probe=12)
        add("sorted_lists", 64, 300, A, src="fused", ds=2, distance=("euclidean", "inner")[r % 2], n_probe=12)
        add("sorted_lists", 128, 300, A, modes[r % 3], n_split=(1, 3)[r % 2], n_probe=12)
    add("pools", 32, 300, FAR_RUNG, src="fused", ds=4, n_probe=12)
    add("sorted_lists", 64, 300, FAR_RUNG, src="fused", ds=2, n_probe=12, n_split=3)
    # large batches: the fp32 table of the short codes (a caller's table rides the route behind long scans only: the
    # hint says so), the 16-bit table at m = 64 (four waves; eight waves at k > 248 behind long cells)
    for m, ds in ((8, 16), (16, 8), (32, 4)):
        for r, A in enumerate(L):
            add("dump_f32", m, (100, 10, 1, 100)[r], A, src="fused", ds=ds, distance=("euclidean", "inner")[r % 2],
                nq=1100)
        add("dump_f32", m, 100, FAR_RUNG, src="fused", ds=ds, nq=1100)
    for r, A in enumerate(L):
        add("dump_f32", 16, (10, 100)[r % 2], A, modes[r % 3], nq=1024, hint=32 * 977)
    for distance in ("euclidean", "inner"):
        if distance == "euclidean":
            add("dump_sel16", 64, 10, FAR_RUNG, src="fused", ds=2, nq=1100)
            add("dump_sel16_w8", 64, 300, FAR_RUNG, src="fused", ds=2, nq=1100, n_probe=12, hint=32 * 977)
        for r, A in enumerate(L):
            add("dump_sel16", 64, (100, 10, 1, 100)[r], A, src="fused", ds=2, distance=distance, nq=1100)
            add("dump_sel16_w8", 64, 300, A, src="fused", ds=(2, 1)[r % 2], distance=distance, nq=1100, n_probe=12,
                hint=32 * 977)
    # the control that is exact by construction: the reference layout (no scan-layout copy; m = 36 has no such kernel)
    for m, k in ((64, 100), (36, 10)):
        for mode in modes:
            add("reference_layout", m, k, L[-1], mode, n_split=(1, 3)[m == 36], packed=m == 36)
    return out


# What was seen for these very inputs (seeded by the case's id).  _DISAGREE: on the CPU, the chain and the pairwise sum
# pick different top-k members for at least one examined query.  On the MI355X: _HELD -- one of those, and no query was
# redone (the band held the right candidates); _REDONE -- at least a fifth of the queries went to the exact kernel.
_DISAGREE = frozenset((
    "dump_f32-m16-k100-s1-fused-euc8-A30",
    "dump_f32-m16-k100-s1-lut-far-A20",
    "dump_f32-m32-k100-s1-fused-euc4-A30",
    "dump_f32-m8-k100-s1-fused-euc16-A30",
    "dump_sel16-m64-k10-s1-fused-euc2-A30",
    "dump_sel16-m64-k100-s1-fused-euc2-A20",
    "dump_sel16_w8-m64-k300-s1-fused-euc1-A20",
    "dump_sel16_w8-m64-k300-s1-fused-euc2-A14",
    "dump_sel16_w8-m64-k300-s1-fused-euc2-A30",
    "one_launch_finish-m12-k10-s1-lut-cancel-A20-t25",
    "one_launch_finish-m128-k10-s1-fused-euc1-A14",
    "one_launch_finish-m128-k10-s1-fused-euc1-A30",
    "one_launch_finish-m128-k10-s3-lut-cancel-A14",
    "one_launch_finish-m128-k100-s1-lut-mixed-A20-t25",
    "one_launch_finish-m128-k100-s3-fused-euc1-A20",
    "one_launch_finish-m16-k10-s1-fused-euc2-A30",
    "one_launch_finish-m32-k1-s1-lut-far-A20-t25",
    "one_launch_finish-m64-k10-s1-fused-euc2-A30",
    "one_launch_finish-m64-k10-s3-lut-cancel-A20-t25",
    "one_launch_finish-m64-k100-s1-lut-far-A10",
    "one_launch_finish-m64-k100-s1-lut-far-A14",
    "one_launch_finish-m64-k100-s1-lut-far-A20",
    "one_launch_finish-m64-k100-s1-lut-mixed-A20",
    "one_launch_finish-m64-k100-s3-fused-euc2-A20",
    "one_launch_finish-m64-k100-s3-lut-cancel-A14",
    "one_launch_finish-m64-k100-s3-lut-cancel-A20",
    "one_launch_finish-m8-k1-s3-lut-far-A20-t25",
    "one_launch_finish-m8-k10-s1-lut-far-A14",
    "one_launch_finish-m8-k10-s1-lut-far-A20",
    "one_launch_finish-m8-k10-s3-lut-cancel-A20",
    "pools-m16-k300-s3-lut-far-A20",
    "pools-m32-k300-s1-fused-euc4-A30",
    "pools-m32-k300-s3-lut-cancel-A10",
    "pools-m32-k300-s3-lut-far-A20",
    "pools-m8-k300-s3-lut-far-A20",
    "reference_layout-m36-k10-s3-lut-cancel-A20",
    "reference_layout-m36-k10-s3-lut-far-A20",
    "reference_layout-m36-k10-s3-lut-mixed-A20",
    "reference_layout-m64-k100-s1-lut-cancel-A20-nopack",
    "reference_layout-m64-k100-s1-lut-far-A20-nopack",
    "reference_layout-m64-k100-s1-lut-mixed-A20-nopack",
    "sorted_lists-m128-k300-s3-lut-cancel-A10",
    "sorted_lists-m128-k300-s3-lut-far-A20",
    "sorted_lists-m64-k300-s1-lut-cancel-A20",
    "sorted_lists-m64-k300-s3-fused-euc2-A30",
    "sorted_lists-m64-k300-s3-lut-far-A14",
))
_HELD = frozenset((
    "dump_f32-m8-k100-s1-fused-euc16-A30",
    "dump_sel16_w8-m64-k300-s1-fused-euc1-A20",
    "dump_sel16_w8-m64-k300-s1-fused-euc2-A14",
    "one_launch_finish-m128-k10-s1-fused-euc1-A14",
    "one_launch_finish-m16-k10-s1-fused-euc2-A30",
    "one_launch_finish-m64-k100-s3-fused-euc2-A20",
    "one_launch_finish-m8-k10-s1-lut-far-A14",
    "pools-m16-k300-s3-lut-far-A20",
    "pools-m32-k300-s1-fused-euc4-A30",
    "pools-m32-k300-s3-lut-cancel-A10",
    "pools-m32-k300-s3-lut-far-A20",
    "pools-m8-k300-s3-lut-far-A20",
))
_REDONE = frozenset((
    "dump_f32-m16-k100-s1-fused-euc8-A30",
    "dump_f32-m16-k100-s1-lut-far-A20",
    "dump_f32-m32-k100-s1-fused-euc4-A30",
    "dump_sel16-m64-k10-s1-fused-euc2-A30",
    "dump_sel16-m64-k100-s1-fused-euc2-A20",
    "dump_sel16_w8-m64-k300-s1-fused-euc2-A30",
    "one_launch_finish-m12-k10-s1-lut-cancel-A20-t25",
    "one_launch_finish-m128-k10-s1-fused-euc1-A30",
    "one_launch_finish-m128-k10-s3-lut-cancel-A14",
    "one_launch_finish-m128-k100-s1-lut-mixed-A20-t25",
    "one_launch_finish-m128-k100-s3-fused-euc1-A20",
    "one_launch_finish-m32-k1-s1-lut-far-A20-t25",
    "one_launch_finish-m64-k1-s1-lut-far-A14",
    "one_launch_finish-m64-k10-s1-fused-euc2-A30",
    "one_launch_finish-m64-k10-s3-lut-cancel-A20-t25",
    "one_launch_finish-m64-k100-s1-lut-far-A10",
    "one_launch_finish-m64-k100-s1-lut-far-A14",
    "one_launch_finish-m64-k100-s1-lut-far-A20",
    "one_launch_finish-m64-k100-s3-lut-cancel-A10",
    "one_launch_finish-m64-k100-s3-lut-cancel-A14",
    "one_launch_finish-m64-k100-s3-lut-cancel-A20",
    "one_launch_finish-m8-k1-s3-lut-far-A20-t25",
    "one_launch_finish-m8-k10-s1-lut-far-A20",
    "one_launch_finish-m8-k10-s3-lut-cancel-A20",
    "sorted_lists-m128-k300-s3-lut-cancel-A10",
    "sorted_lists-m128-k300-s3-lut-far-A20",
    "sorted_lists-m64-k300-s1-lut-cancel-A20",
    "sorted_lists-m64-k300-s3-fused-euc2-A30",
    "sorted_lists-m64-k300-s3-lut-far-A14",
))

BAND_CASES = _band_cases()
assert len({c["id"] for c in BAND_CASES}) == len(BAND_CASES)
assert (_DISAGREE | _HELD | _REDONE) <= {c["id"] for c in BAND_CASES} and _HELD <= _DISAGREE and not (_HELD & _REDONE)
for _c in BAND_CASES:
    if _c["id"] in _DISAGREE:
        _c["disagree"] = True
    _c["expect"] = "held" if _c["id"] in _HELD else ("redone" if _c["id"] in _REDONE else None)
