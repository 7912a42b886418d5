"""GPU: the container kernels (csrc/container.hip, csrc/pack.hip -- what CellContainer's add, remove and expand run)
against the plain references of oracle.ivfpq_oracle, at the shapes where such kernels go wrong: the 64-slot steps of the
write-address walk, runs of 2^k and 2^k +- 1 equal labels, zero-capacity cells, block edges of the id search, partial
ranges of the scan-layout pack.  Integer work: every comparison is array_equal.

Labels and cell indices stay inside [0, n_cells): the kernels index the cell tables unchecked."""
import numpy as np
import pytest
import torch

from oracle import ivfpq_oracle as orc
from tests_support import DEV, N, T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def K():
    import torchpq_amd.kernels as k
    from torchpq_amd import _lib
    _lib.load()  # fail loudly if libtorchpq_amd.so is missing
    return k


def _same(got, want):
    got = N(got)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:8]


# ---------------------------------------------------------------------------------------------
# get_ioa
# ---------------------------------------------------------------------------------------------
RUNS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)


def _ioa(K, labels, n_cells):
    labels = np.asarray(labels, np.int64)
    _same(K.GetIOAHip()(T(labels), n_cells=n_cells), orc.get_ioa(labels))


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 513])
def test_get_ioa_sizes_around_a_block(K, n):
    rng = np.random.default_rng(n)
    _ioa(K, rng.integers(0, 3, n), 3)
    _ioa(K, rng.integers(0, 300, n), 300)


def test_get_ioa_one_label_for_the_whole_array(K):
    _ioa(K, np.zeros(5000), 1)
    _ioa(K, np.full(5000, 6), 7)
    _ioa(K, np.full(5000, 6), None)


@pytest.mark.parametrize("order", ["shuffled", "sorted"])
def test_get_ioa_runs_of_powers_of_two_and_their_neighbours(K, order):
    """every run length 2^k - 1, 2^k, 2^k + 1 the gallop and the binary search can meet; the longest run belongs to the
    smallest label, so it starts at sorted index 0"""
    rng = np.random.default_rng(5)
    lengths = np.array(RUNS[::-1])                                        # label 0: 1025 of them
    lengths[1:] = rng.permutation(lengths[1:])
    labels = np.repeat(np.arange(len(RUNS)), lengths)
    assert np.bincount(labels)[0] == max(RUNS) and sorted(np.bincount(labels)) == list(RUNS)
    if order == "shuffled":
        labels = rng.permutation(labels)
    _ioa(K, labels, len(RUNS))
    _ioa(K, labels, None)


@pytest.mark.parametrize("c", [1, 2, 3, 64])
def test_get_ioa_round_robin_labels(K, c):
    _ioa(K, np.arange(1000) % c, c)


@pytest.mark.parametrize("n_cells", [1, 2, 3, 4, 5, 1024, 1025])
def test_get_ioa_sort_bits_cover_the_top_label(K, n_cells):
    rng = np.random.default_rng(n_cells)
    labels = rng.integers(0, n_cells, 700)
    labels[[0, 350, 699]] = n_cells - 1
    labels[[1, 698]] = 0
    # with one sort bit too few the top label would sort as label 0 (1024 = 2^10, 4 = 2^2): mix the two
    labels[100:140] = np.where(np.arange(40) % 2 == 0, n_cells - 1, 0)
    assert labels.min() >= 0 and labels.max() == n_cells - 1
    _ioa(K, labels, n_cells)


def test_get_ioa_all_key_bits_without_n_cells(K):
    rng = np.random.default_rng(6)
    values = np.array([0, 1, 2 ** 16, 2 ** 30, 2 ** 30 + 1, 1_999_999_999, 2_000_000_000], np.int64)
    _ioa(K, values[rng.integers(0, len(values), 3000)], None)
    _ioa(K, rng.integers(0, 2_000_000_001, 3000), None)


# ---------------------------------------------------------------------------------------------
# get_write_address
# ---------------------------------------------------------------------------------------------
WA_CAP = np.array([0, 1, 63, 64, 65, 127, 128, 129, 200, 300], np.int64)
WA_START = np.cumsum(WA_CAP) - WA_CAP                                       # back to back: starts are not 64-aligned
WA_PATTERNS = ("all", "none", "first", "last", "upper_half_lanes", "third_step", "alternating", "random")


def _wa_is_empty(pattern):
    rng = np.random.default_rng(12)
    out = np.zeros(int(WA_CAP.sum()), np.uint8)
    for st, cap in zip(WA_START.tolist(), WA_CAP.tolist()):
        r = np.arange(cap)                                                   # position inside the cell
        free = {"all": r >= 0, "none": r < 0, "first": r == 0, "last": r == cap - 1, "upper_half_lanes": r % 64 >= 32,
                "third_step": (r >= 128) & (r < 192), "alternating": r % 2 == 1, "random": rng.random(cap) < 0.5}[pattern]
        out[st:st + cap] = free
    return out


def _wa_queries(is_empty, seed=0):
    """(cell, rank) for every cell and every rank 0 .. n_free - 1, then n_free and n_free + 5 (both: no such slot), in
    random order so that the four waves of a block serve different cells"""
    n_slots = is_empty.shape[0]
    cells, ranks = [], []
    for c, (st, cap) in enumerate(zip(WA_START.tolist(), WA_CAP.tolist())):
        n_free = int(is_empty[st:min(st + cap, n_slots)].sum())
        r = list(range(n_free)) + [n_free, n_free + 5]
        cells += [c] * len(r)
        ranks += r
    order = np.random.default_rng(seed).permutation(len(cells))
    return np.array(cells, np.int64)[order], np.array(ranks, np.int64)[order]


def _wa(K, is_empty, cells, ranks):
    want = orc.get_write_address(is_empty, WA_START, WA_CAP, cells, ranks)
    _same(K.GetWriteAddressHip()(T(is_empty), T(WA_START), T(WA_CAP), T(cells), T(ranks)), want)
    return want


@pytest.mark.parametrize("pattern", WA_PATTERNS)
def test_get_write_address_every_rank_of_every_cell(K, pattern):
    is_empty = _wa_is_empty(pattern)
    cells, ranks = _wa_queries(is_empty)
    want = _wa(K, is_empty, cells, ranks)
    # what the oracle says is what the pattern means: every free slot of every cell is handed out exactly once
    assert sorted(want[want >= 0].tolist()) == np.nonzero(is_empty)[0].tolist()
    assert (want < 0).sum() == 2 * len(WA_CAP)


def test_get_write_address_clips_the_last_cell_to_the_array(K):
    for pattern in ("all", "random", "last"):
        is_empty = _wa_is_empty(pattern)[:-37]                               # the last cell: 263 of its 300 slots exist
        cells, ranks = _wa_queries(is_empty, seed=1)
        want = _wa(K, is_empty, cells, ranks)
        assert want.max() < is_empty.shape[0]
        assert sorted(want[want >= 0].tolist()) == np.nonzero(is_empty)[0].tolist()


@pytest.mark.parametrize("n_labels", [1, 3, 4, 5])
def test_get_write_address_label_counts_around_a_block_of_four(K, n_labels):
    is_empty = _wa_is_empty("random")
    cells, ranks = _wa_queries(is_empty, seed=2)
    keep = np.nonzero(WA_CAP[cells] >= 127)[0][:n_labels]                    # long cells: several steps per wave
    want = _wa(K, is_empty, cells[keep], ranks[keep])
    assert want.shape == (n_labels,)


# ---------------------------------------------------------------------------------------------
# get_cell_by_address, get_id_by_address
# ---------------------------------------------------------------------------------------------
def _layout(cap, start=None):
    cap = np.array(cap, np.int64)
    start = np.cumsum(cap) - cap if start is None else np.array(start, np.int64)
    assert (np.diff(start) >= 0).all() and (start[1:] >= (start + cap)[:-1]).all()
    return start, cap


CELL_LAYOUTS = {
    "one_cell": _layout([10]),
    "one_cell_off_zero": _layout([5], [3]),
    "zero_capacity_first_last_and_a_run": _layout([0, 0, 5, 3, 0, 0, 0, 0, 0, 7, 1, 0]),
    "all_zero_but_one": _layout([0, 0, 0, 9, 0, 0]),
    "all_zero_but_the_first": _layout([4, 0, 0, 0]),
    "all_zero_but_the_last": _layout([0, 0, 0, 4]),
    "gaps": _layout([3, 0, 5, 4, 0, 6], [2, 10, 10, 30, 40, 41]),
    "many": _layout(np.random.default_rng(2).integers(0, 4, 300) * np.random.default_rng(3).integers(0, 40, 300)),
}
EXTREME = [-2 ** 40, -1, 0, 2 ** 40]


def _edge_addresses(start, cap, count):
    end = start + cap
    total = int(end.max())
    edges = np.concatenate([start - 1, start, end - 1, end, EXTREME, [total, total + 1]]).astype(np.int64)
    rng = np.random.default_rng(count)
    if len(edges) < count:
        edges = np.concatenate([edges, rng.integers(-3, total + 4, count - len(edges))])
    else:   # ("many" only) a sample of its 1200 edges, every extreme kept; ..._every_address_of_the_layouts has them all
        edges = np.concatenate([edges[-6:], rng.permutation(edges[:-6])[:count - 6]])
    return rng.permutation(edges)


@pytest.mark.parametrize("name", list(CELL_LAYOUTS))
def test_get_cell_by_address_at_every_cell_edge(K, name):
    start, cap = CELL_LAYOUTS[name]
    for count in (255, 256, 257):
        adr = _edge_addresses(start, cap, count)
        assert adr.shape == (count,) and {-2 ** 40, 2 ** 40}.issubset(adr.tolist())
        want = orc.get_cell_by_address(adr, start, cap)
        _same(K.GetCellByAddressHip()(T(adr), T(start), T(start + cap)), want)
        assert (cap[want[want >= 0]] > 0).all() and (want >= 0).sum() >= min(3, int(cap.sum()))


def test_get_cell_by_address_every_address_of_the_layouts(K):
    for start, cap in CELL_LAYOUTS.values():
        adr = np.arange(-2, int((start + cap).max()) + 3, dtype=np.int64)
        _same(K.GetCellByAddressHip()(T(adr), T(start), T(start + cap)), orc.get_cell_by_address(adr, start, cap))


def test_get_id_by_address_extremes_and_shapes(K):
    rng = np.random.default_rng(14)
    for cap in (1, 255, 256, 257, 1000):
        a2i = rng.integers(-1, 2 ** 62, cap)
        a2i[rng.random(cap) < 0.3] = -1
        adr = np.concatenate([EXTREME, [cap - 1, cap, cap + 1], rng.integers(-3, cap + 3, 257 * 3 - 7)]).astype(np.int64)
        for shape in ((-1,), (3, 257), (257, 3), (1, 3, 257)):
            probe = rng.permutation(adr).reshape(shape)
            _same(K.GetIdByAddressHip()(T(a2i), T(probe)), orc.get_id_by_address(a2i, probe))


# ---------------------------------------------------------------------------------------------
# get_address_by_id: the linear search, and the container's three paths
# ---------------------------------------------------------------------------------------------
def _id_table(cap, id_scale, seed):
    """address -> id with free addresses (-1) and ids stored two and three times, their copies at least 5000 addresses
    apart where the capacity allows (so different blocks of the search see them); returns (table, repeated ids)"""
    rng = np.random.default_rng(seed)
    a2i = rng.permutation(max(cap, 1) * 4)[:cap].astype(np.int64) * id_scale + 1   # distinct
    a2i[rng.random(cap) < 0.3] = -1
    gap = 5000 if cap > 10000 else cap // 3
    repeated = []
    if gap >= 1:
        for t, a in enumerate(rng.permutation(min(gap, cap - 2 * gap))[:40].tolist()):
            copies = (a, a + gap, a + 2 * gap) if t % 2 else (a, a + 2 * gap)
            a2i[list(copies)] = (4 * cap + 7 + t) * id_scale                        # no other address holds it
            repeated.append(int(a2i[a]))
    return a2i, np.array(repeated, np.int64)


def _id_queries(a2i, repeated, n_ids, seed):
    """present ids (the repeated ones first), absent ids, -1, -5, 2^62, ids asked for twice"""
    rng = np.random.default_rng(seed)
    present = a2i[a2i >= 0]
    rest = rng.permutation(np.concatenate([rng.permutation(present)[:n_ids], rng.integers(0, 2 ** 40, n_ids)]))
    pool = np.concatenate([repeated[:6], [-1, -5, 2 ** 62, 0, 2], repeated[:3], present[:8], present[:3] + 1,
                           repeated[6:], rest]).astype(np.int64)
    q = pool[:n_ids]
    return np.concatenate([q[:11], rng.permutation(q[11:])])


ID_CAPACITIES = [0, 1, 255, 256, 257, 4096, 4097, 8193, 20000]
ID_COUNTS = [0, 1, 255, 256, 257, 600]


@pytest.mark.parametrize("cap", ID_CAPACITIES)
def test_get_address_by_id_linear_search(K, cap):
    a2i, repeated = _id_table(cap, 3, cap)
    assert cap < 3 or len(repeated) >= min(40, cap // 3) // 2
    if cap > 10000:
        first = np.array([np.nonzero(a2i == r)[0] for r in repeated[1::2]])
        assert first.shape[1] == 3 and (np.diff(first, axis=1) >= 5000).all()
    dev = T(a2i)
    for n_ids in ID_COUNTS:
        ids = _id_queries(a2i, repeated, n_ids, n_ids)
        assert ids.shape == (n_ids,)
        want = orc.get_address_by_id(a2i, ids)
        _same(K.GetAddressByIdHip()(dev, T(ids)), want)
        if cap >= 255 and n_ids >= 255:
            assert (want >= 0).sum() > 10 and (want < 0).sum() > 10


def _bare_container(a2i, use_inverse_id_mapping):
    from torchpq_amd.container.BaseContainer import BaseContainer

    class Bare(BaseContainer):
        def add(self):
            pass

        def remove(self):
            pass

    c = Bare(device=DEV, initial_size=a2i.shape[0], use_inverse_id_mapping=use_inverse_id_mapping)
    c._address2id.copy_(T(a2i))
    c._max_id = int(a2i.max())
    return c


@pytest.mark.parametrize("path", ["linear", "dense_table", "sorted_list"])
def test_container_id_paths_return_the_smallest_address(K, path):
    """BaseContainer.get_address_by_id on a table with ids stored several times (reference-built indexes have them):
    every path answers with the smallest address holding the id, as the oracle does -- remove(ids=...) then removes the
    same copy whatever the container's settings"""
    cap = 20000
    scale = 1 if path != "sorted_list" else 1 << 14                            # sparse: max_id + 1 > 8 cap + 2^20
    a2i, repeated = _id_table(cap, scale, 77)
    rng = np.random.default_rng(78)
    # many more repeats, close together and far apart, on top of the planted ones
    for t in range(3000):
        src, dst = rng.integers(0, cap, 2)
        if a2i[src] >= 0:
            a2i[dst] = a2i[src]
    ids_u, counts = np.unique(a2i[a2i >= 0], return_counts=True)
    assert (counts >= 2).sum() > 1000 and (counts >= 3).sum() > 20
    c = _bare_container(a2i, path != "linear")
    ids = np.concatenate([ids_u, repeated, [-1, -5, 0, 2 ** 62, int(a2i.max()) + 1], ids_u[:50] + 1])
    ids = rng.permutation(ids).astype(np.int64)
    want = orc.get_address_by_id(a2i, ids)
    got = c.get_address_by_id(T(ids))
    assert (c._id2address is not None, c._sparse_id_map is not None) == (path == "dense_table", path == "sorted_list")
    _same(got, want)
    _same(c.get_address_by_id(T(ids[:35].reshape(7, 5))), want[:35].reshape(7, 5))


# ---------------------------------------------------------------------------------------------
# grow_cells
# ---------------------------------------------------------------------------------------------
GROW_LAYOUTS = {
    # old capacity 0 -> positive, cells that do not grow, new capacity 0, 700 slots: three trips of the 256-stride loop
    "mixed": ([0, 5, 300, 0, 64, 10, 3, 256, 0, 1], [9, 5, 700, 0, 64, 257, 4, 256, 1, 1]),
    "grid_y_2": ([3000, 0, 2], [7000, 0, 5]),                                # (7005 / 3 + 2047) / 2048 = 2 block rows
    "nearly_nothing_stored": ([0, 2, 0], [4, 2, 300]),
    "one_cell": ([255], [513]),
}


@pytest.mark.parametrize("g", [1, 2, 3, 16])
@pytest.mark.parametrize("name", list(GROW_LAYOUTS))
def test_grow_cells_moves_every_cell_and_frees_the_new_tails(K, g, name):
    rng = np.random.default_rng(g * 100 + len(name))
    old_cap, new_cap = (np.array(x, np.int64) for x in GROW_LAYOUTS[name])
    old_start, new_start = np.cumsum(old_cap) - old_cap, np.cumsum(new_cap) - new_cap
    old_slots, new_slots = int(old_cap.sum()), int(new_cap.sum())
    storage = rng.integers(1, 256, (g, old_slots, 4), dtype=np.uint8)       # no zero byte: a zeroed tail is told apart
    is_empty = (rng.random(old_slots) < 0.3).astype(np.uint8)                # tombstones keep their stale codes
    a2i = np.where(is_empty == 1, -1, rng.permutation(old_slots * 3)[:old_slots] + 1).astype(np.int64)
    want = orc.grow_cells(storage, a2i, is_empty, old_start, old_cap, new_start, new_cap, new_slots)
    args = [T(x) for x in (storage, a2i, is_empty, old_start, old_cap, new_start, new_cap)]
    out = (torch.full((g, new_slots, 4), 0xCD, device=DEV, dtype=torch.uint8),
           torch.full((new_slots,), -7, device=DEV, dtype=torch.int64),
           torch.full((new_slots,), 0xCD, device=DEV, dtype=torch.uint8))
    got = K.GrowCellsHip()(*args, new_slots, out=out)
    for a, b, e in zip(got, out, want):
        assert a.data_ptr() == b.data_ptr()
        _same(a, e)
    for a, e in zip(K.GrowCellsHip()(*args, new_slots, out=None), want):
        _same(a, e)
    for a, e in zip(args, (storage, a2i, is_empty, old_start, old_cap, new_start, new_cap)):
        _same(a, e)                                                          # the inputs are read only


# ---------------------------------------------------------------------------------------------
# pack_codes, scatter_codes
# ---------------------------------------------------------------------------------------------
PACK_M = [4, 8, 12, 16, 24, 32, 64, 96, 120]
PACK_SLOTS = 333


def _pack_case(m):
    storage = np.random.default_rng(m).integers(0, 256, (m // 4, PACK_SLOTS, 4), dtype=np.uint8)
    return storage, orc.pack_codes(storage)


@pytest.mark.parametrize("m", PACK_M)
def test_pack_codes_equals_the_documented_layout(K, m):
    storage, want = _pack_case(m)
    _same(K.PackCodesHip()(T(storage)), want)
    st = T(storage)
    for begin, end in [(0, 0), (0, 1), (332, 333), (37, 38), (5, 300), (333, 333), (63, 65), (0, 333)]:
        buf = torch.full(want.shape, 0xEE, device=DEV, dtype=torch.uint8)
        assert K.PackCodesHip()(st, buf, begin, end) is buf
        expect = np.full_like(want, 0xEE)
        expect[:, begin:end] = want[:, begin:end]                            # packed [m/W][slot][W]: a slot range is axis 1
        _same(buf, expect)
    _same(st, storage)


def test_pack_codes_argument_errors(K):
    from torchpq_amd._lib import TorchPQAmdError, check, load, ptr
    st = T(_pack_case(8)[0])
    buf = torch.full((1, PACK_SLOTS, 8), 0xEE, device=DEV, dtype=torch.uint8)
    for begin, end in [(5, 3), (0, PACK_SLOTS + 1), (-1, 4), (PACK_SLOTS + 1, PACK_SLOTS + 1)]:
        with pytest.raises(TorchPQAmdError, match="bad slot range"):
            K.PackCodesHip()(st, buf, begin, end)
    for m in (6, 0, -4):
        with pytest.raises(TorchPQAmdError, match="multiple of 4"):
            check(load().tpq_ivfpq_pack_codes(ptr(st), ptr(buf), PACK_SLOTS, m, 0, PACK_SLOTS, None), "tpq_ivfpq_pack_codes")
    torch.cuda.synchronize()
    assert bool((buf == 0xEE).all())                                         # a refused call writes nothing


@pytest.mark.parametrize("m", PACK_M)
def test_scatter_codes_keeps_the_packed_copy_in_step(K, m):
    """ScatterCodesHip with a scan-layout copy: both arrays end as scatter-then-full-pack; addresses outside the array,
    repeated, are skipped (the valid ones are distinct: two writers of one slot would race)"""
    rng = np.random.default_rng(m + 1)
    storage, packed = _pack_case(m)
    n = 257
    codes = rng.integers(0, 256, (m, n), dtype=np.uint8)
    adr = rng.permutation(PACK_SLOTS)[:n].astype(np.int64)
    adr[rng.permutation(n)[:40]] = np.resize(np.array([-1, -1, PACK_SLOTS, PACK_SLOTS + 4, -2 ** 40, 2 ** 40, -1]), 40)
    assert len(set(adr[(adr >= 0) & (adr < PACK_SLOTS)].tolist())) == ((adr >= 0) & (adr < PACK_SLOTS)).sum()
    st, pk = T(storage), T(packed)
    K.ScatterCodesHip()(T(codes), T(adr), st, pk)
    orc.codes_to_storage(codes, adr, storage)
    _same(st, storage)
    _same(pk, orc.pack_codes(storage))
    st2 = T(_pack_case(m)[0])
    K.ScatterCodesHip()(T(codes), T(adr), st2)                               # without the copy: storage alone
    _same(st2, storage)


# ---------------------------------------------------------------------------------------------
# pq_decode
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,ds,n", [(1, 1, 1), (4, 7, 255), (8, 4, 256), (16, 1, 257), (64, 2, 1000)])
def test_pq_decode_is_an_exact_gather(K, m, ds, n):
    rng = np.random.default_rng(m * n)
    cb = rng.standard_normal((m, ds, 256)).astype(np.float32)
    cb[0, 0, :3] = [np.float32(-0.0), np.float32(1e-45), np.float32(3.4e38)]   # moved as bits, not as values
    codes = rng.integers(0, 256, (m, n), dtype=np.uint8)
    codes[:, 0], codes[:, -1] = 0, 255
    got = N(K.PQDecodeHip()(T(cb), T(codes)))
    want = orc.pq_decode(cb, codes)
    assert got.shape == want.shape == (m * ds, n) and got.dtype == np.float32
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
