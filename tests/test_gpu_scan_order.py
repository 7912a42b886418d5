"""GPU: the dispatch order of the large-batch scan routes (csrc/scan_order.hip).

tpq_ivfpq_scan_order alone against numpy -- the work per query with the clamps of the scan's own probe table, the order a
permutation with the work non-increasing and equal work in query order, the rank its inverse -- and the packed scan
end to end on a skewed index at batch sizes just past the chip's workgroup slots, against the C oracle bit for bit, with
the order on and -- the caller's workspace sized to the lists in use alone -- off."""
import numpy as np
import pytest
import torch

from oracle import c_oracle
from oracle import ivfpq_oracle as orc
from test_gpu_kernels import _random_index, T, N

pytestmark = pytest.mark.gpu


# ---- the ordering kernels alone ---------------------------------------------------------------------------------------
def _work(cs, sz, npl, shift):
    """the tiles a query scans, as fetch_probes / build_probe_table (csrc/scan_shared.h) count them"""
    nq, mp = cs.shape
    n = np.clip(npl, 0, mp)
    size = np.maximum(sz, 0)
    size[:, 1:][cs[:, 1:] == cs[:, :-1]] = 0                  # a cell listed twice in a row is scanned once
    size[np.arange(mp)[None, :] >= n[:, None]] = 0
    return ((size + (1 << shift) - 1) >> shift).sum(1)


def _order_inputs(rng, nq, mp, equal):
    if equal:   # every query the same work, from different rows
        sz = np.tile(rng.integers(1, 300, mp), (nq, 1))
        cs = np.cumsum(np.full((nq, mp), 400), 1) + rng.integers(0, 50, (nq, 1))
        return cs.astype(np.int64), sz.astype(np.int64), np.full(nq, mp, np.int64)
    sz = rng.integers(-40, 900, (nq, mp))
    sz[rng.random((nq, mp)) < 0.1] = 0
    sz[rng.random((nq, mp)) < 0.02] = rng.integers(5000, 60000)     # a few long cells: uneven work
    cs = rng.integers(0, 1 << 20, (nq, mp))
    if mp > 1:                                                      # rows with repeated starts
        rep = rng.random((nq, mp - 1)) < 0.15
        cs[:, 1:][rep] = cs[:, :-1][rep]
    npl = rng.integers(-2, mp + 3, nq)                              # 0, negatives, values above max_nprobe
    npl[: min(nq, 3)] = (0, -1, mp + 5)[: min(nq, 3)]
    return cs.astype(np.int64), sz.astype(np.int64), npl.astype(np.int64)


@pytest.mark.parametrize("nq", [1, 63, 1025, 20000])
@pytest.mark.parametrize("mp", [1, 8, 70])
@pytest.mark.parametrize("shift", [6, 8])
def test_order_is_longest_first(nq, mp, shift):
    import torchpq_amd.kernels as K
    rng = np.random.default_rng(nq * 100 + mp + shift)
    cs, sz, npl = _order_inputs(rng, nq, mp, equal=False)
    order, rank, work = (N(t) for t in K.ScanOrderHip()(T(cs), T(sz), T(npl), shift))
    want = _work(cs, sz, npl, shift)
    assert np.array_equal(work, want)
    assert np.array_equal(np.sort(order), np.arange(nq))                         # a permutation
    assert np.array_equal(rank[order], np.arange(nq))                            # rank is its inverse
    w = want[order]
    # for every i < j: work[order[i]] >= work[order[j]] - max(work) / 64
    assert (np.minimum.accumulate(w)[:-1] >= w[1:] - want.max() / 64).all()
    # (the kernel ranks exactly: non-increasing work, equal work by ascending query)
    assert np.array_equal(order, np.lexsort((np.arange(nq), -want)))


@pytest.mark.parametrize("nq,mp", [(1025, 8), (20000, 70)])
def test_equal_work_keeps_query_order(nq, mp):
    import torchpq_amd.kernels as K
    rng = np.random.default_rng(nq + mp)
    cs, sz, npl = _order_inputs(rng, nq, mp, equal=True)
    order, rank, work = (N(t) for t in K.ScanOrderHip()(T(cs), T(sz), T(npl), 6))
    assert (work == work[0]).all() and work[0] == _work(cs, sz, npl, 6)[0] > 0
    assert np.array_equal(order, np.arange(nq)) and np.array_equal(rank, np.arange(nq))


# ---- end to end on the packed scan ----------------------------------------------------------------------------------
N_PROBE = 8


def _slots():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count   # four scan workgroups per CU


class _Skewed:
    """a skewed index -- most cells 10 - 60 slots, a few of 1 500 - 2 000 -- with its queries, probes and the oracle's
    answers for k = 100 and k = 1, built once per m; a batch of nq queries is the first nq of them"""

    def __init__(self, m, nq, ks):
        rng = np.random.default_rng(640 + m)
        n_cells, ds = 160, 2
        sizes = rng.integers(10, 61, n_cells)
        sizes[rng.choice(n_cells, 6, replace=False)] = rng.integers(1500, 2001, 6)
        self.storage, self.is_empty, start, sizes, self.a2i = _random_index(rng, m, n_cells, 0, 40, 0.0, sizes=sizes)
        self.codebook = rng.standard_normal((m, ds, 256)).astype(np.float32)
        self.query = rng.standard_normal((m * ds, nq)).astype(np.float32)
        cells = np.stack([rng.permutation(n_cells)[:N_PROBE] for _ in range(nq)])
        self.npl = rng.integers(0, N_PROBE + 1, nq).astype(np.int64)            # per-query probe counts, 0 included
        self.npl[::3] = N_PROBE
        self.cs, self.sz = start[cells], sizes[cells]
        lut = c_oracle.adc_lut(self.query, self.codebook, "euclidean")
        self.want = {}
        for k in ks:
            ev, ea = c_oracle.scan_topk(self.storage, lut, self.is_empty, self.cs, self.sz, self.npl, k)
            self.want[k] = (ev, ea, orc.get_id_by_address(self.a2i, ea))
        self.m, self.nq = m, nq
        self.dev = None

    def run(self, K, nq, k, workspace_bytes=None):
        if self.dev is None:
            st = T(self.storage)
            self.dev = (st, K.PackCodesHip()(st), T(self.codebook), T(self.is_empty), T(self.a2i))
        st, packed, codebook, is_empty, a2i = self.dev
        scan = K.IVFPQTopkHip(m=self.m)
        scan.workspace_bytes = workspace_bytes
        out = scan.topk_fused(st, T(self.query[:, :nq]), codebook, is_empty, T(self.cs[:nq]), T(self.sz[:nq]),
                              T(self.npl[:nq]), k, packed=packed, address2id=a2i)
        return scan, [N(t) for t in out]


@pytest.fixture(scope="module")
def skewed64():
    return _Skewed(64, 2 * _slots() + 600, (100, 1))


@pytest.fixture(scope="module")
def skewed32():
    return _Skewed(32, _slots() + 76, (100,))


def _lists_in_use(scan):
    """bytes of the last call's workspace its flags, bands and candidate lists take: the order needs three int32 per
    query, each array rounded up to 256 bytes, behind them -- the smallest workspace the library orders the call with,
    less that (tpq_ivfpq_scan_ordered is a host function: nothing is launched)"""
    nq = scan.last_call["n_query"]
    lo, hi = 0, scan.last_workspace_bytes
    assert scan.ordered(hi) and not scan.ordered(lo)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (lo, mid) if scan.ordered(mid) else (mid, hi)
    return hi - 3 * ((nq * 4 + 255) // 256 * 256)


def _check(K, idx, nq, k, route):
    scan, got = idx.run(K, nq, k)
    assert scan.last_route() == route and scan.last_ordered() is True
    for g, w in zip(got, idx.want[k]):
        assert np.array_equal(g, w[:nq])                      # values bit-equal, addresses and ids equal
    # the same call with a workspace that holds the lists in use and nothing else: index order, same bits
    exact = _lists_in_use(scan)
    plain, again = idx.run(K, nq, k, workspace_bytes=exact)
    assert plain.last_route() == route and plain.last_ordered() is False
    for g, a in zip(got, again):
        assert np.array_equal(g.view(np.int32) if g.dtype == np.float32 else g,
                              a.view(np.int32) if a.dtype == np.float32 else a)


@pytest.mark.parametrize("extra", ["slots+76", "2*slots", "2*slots+452", "2*slots+600"])
def test_ordered_scan_equals_the_oracle(skewed64, extra):
    """a split tail under the order, exact rounds, ragged last rounds: one the split rule still deals in two parts on a
    chip of 1 024 slots, one (more than half a round left over) it keeps whole"""
    import torchpq_amd.kernels as K
    slots = _slots()
    nq = {"slots+76": slots + 76, "2*slots": 2 * slots, "2*slots+452": 2 * slots + 452,
          "2*slots+600": 2 * slots + 600}[extra]
    _check(K, skewed64, nq, 100, "dump_sel16")


def test_ordered_scan_at_k_1(skewed64):
    """k = 1: lists of one register.  A ragged round kept whole leaves room for the order; a tail dealt in four parts
    uses the 16 one-register lists per query the workspace size covers at k <= 56 -- no room behind them, index order"""
    import torchpq_amd.kernels as K
    _check(K, skewed64, 2 * _slots() + 600, 1, "dump_sel16")
    nq = _slots() + 76
    scan, got = skewed64.run(K, nq, 1)
    assert scan.last_route() == "dump_sel16" and scan.last_ordered() is False
    for g, w in zip(got, skewed64.want[1]):
        assert np.array_equal(g, w[:nq])


def test_ordered_scan_on_the_f32_route(skewed32):
    import torchpq_amd.kernels as K
    _check(K, skewed32, _slots() + 76, 100, "dump_f32")


def test_a_batch_of_one_round_is_not_ordered(skewed64):
    import torchpq_amd.kernels as K
    scan, got = skewed64.run(K, _slots(), 100)
    assert scan.last_route() == "dump_sel16" and scan.last_ordered() is False
    for g, w in zip(got, skewed64.want[100]):
        assert np.array_equal(g, w[:_slots()])
