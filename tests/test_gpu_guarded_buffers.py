"""GPU: every entry point of the library under guarded, pre-filled allocations (tests/guarded_alloc.py).

The rest of the suite pins WHAT the kernels compute.  This module pins where they write and what they read first: each
case of tests/guarded_cases.py runs its wrapper calls three times -- plainly, then with every torch.empty / empty_like /
zeros of torchpq_amd/kernels/ handed out between two 64-KiB canaries and pre-filled with 0x00, then with 0xFF (every
uncleared counter -1, every uncleared float a NaN) -- and asserts

  * the canaries are intact after both guarded runs: no output and no workspace was written before its first or past
    its last byte (within 64 KiB of it: the harness's blind spot is a wilder write than that);
  * the three results are the same, bit for bit: nothing was read that the call had not written;
  * the route the case is about was the one that ran (scan.last_route(), last_cell_major(), last_cell_norms(),
    last_ordered(), CoarseAssignHip.last_rechecked(), centroid_oracle.route, the split the wrapper reports).

The shapes are the smallest at which the indexing in question exists, ragged on purpose: query counts, k, cell sizes
and the storage capacity are no multiples of the tile, so the last row, list or segment ends inside the buffer's last
partial unit.  The inputs come from the existing generators (test_gpu_kernels._random_index, the *_cases modules, the
oracles' own families); the expected result of a case is its own plain call.

NOT compared bit for bit -- results that depend on the order in which workgroups arrive, held with the existing tests'
own comparison (guarded_cases.NOT_BIT_EXACT has the source lines):

  compute_centroids_*          fp32 sums by unsafeAtomicAdd (csrc/centroid_update.hip:70, :75, :92, :94, :323, :330):
                               test_gpu_centroid_update._check_general on Gaussian data -- and bit for bit on the small
                               integers of centroid_oracle.make_integers_small, which any order sums exactly;
  lloyd_prepare_and_two_steps  the new centroids only (csrc/lloyd.hip:233, :240, :258, :260):
                               test_gpu_lloyd_update.lloyd_bound; maxima and labels bit for bit;
  cell_candidates_*            a query's candidates are appended at an atomic counter (csrc/scan_cells.hip:566):
                               test_gpu_scan_cell_norms._pairs -- the (address, value bits) pairs sorted by address;
                               counts, bands and flags bit for bit.

Everything else is compared bit for bit -- the range fills too (each wave fills its own counted segment in scan order:
the existing range tests compare them entry for entry), and the values the header calls approximate (`vals` of
CoarseAssignHip / MaxSimSelectHip / LloydStepHip): they are functions of the inputs alone.
"""
import contextlib

import numpy as np
import pytest
import torch

import guarded_alloc as ga
import guarded_cases as gc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32, I64, I32, U8 = torch.float32, torch.int64, torch.int32, torch.uint8
BUILDERS = {}


def case(cid):
    def register(build):
        assert cid in gc.CASE_SYMBOLS and cid not in BUILDERS, cid
        BUILDERS[cid] = build
        return build
    return register


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def kernels():
    import torchpq_amd.kernels as K
    from torchpq_amd import _lib
    _lib.load()
    return K


def gempty(*shape, dtype):
    """allocated the way the wrappers allocate: between canaries, pre-filled, while an arena is installed"""
    from torchpq_amd.kernels import _common
    return _common.torch.empty(*shape, device=DEV, dtype=dtype)


def same_bits(a, b, where="result"):
    """the two results are equal bit for bit (NaN payloads and signed zeros included), element by element"""
    if isinstance(a, (tuple, list)):
        assert isinstance(b, (tuple, list)) and len(a) == len(b), where
        for i, (x, y) in enumerate(zip(a, b)):
            same_bits(x, y, f"{where}[{i}]")
    elif isinstance(a, dict):
        assert isinstance(b, dict) and a.keys() == b.keys(), where
        for key in a:
            same_bits(a[key], b[key], f"{where}[{key!r}]")
    elif torch.is_tensor(a):
        assert torch.is_tensor(b) and a.shape == b.shape and a.dtype == b.dtype, (where, a.shape, b.shape)
        x, y = a.contiguous().reshape(-1).view(U8), b.contiguous().reshape(-1).view(U8)
        if not torch.equal(x, y):
            bad = torch.nonzero(x != y).reshape(-1) // a.element_size()
            raise AssertionError(f"{where}: {len(torch.unique(bad))} of {a.numel()} elements differ, first at flat index "
                                 f"{int(bad[0])}: {a.reshape(-1)[int(bad[0])].item()!r} != {b.reshape(-1)[int(bad[0])].item()!r}")
    elif isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and a.shape == b.shape and a.dtype == b.dtype, (where, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8)) // a.itemsize
            raise AssertionError(f"{where}: {len(np.unique(bad))} of {a.size} elements differ, first at flat index "
                                 f"{bad[0]}: {a.reshape(-1)[bad[0]]!r} != {b.reshape(-1)[bad[0]]!r}")
    else:
        assert a == b, (where, a, b)


END_TO_END = ("index_plain_end_to_end", "index_residual_end_to_end")    # (their own test: an arena per index call)


@pytest.fixture(scope="module", autouse=True)
def _totals():
    """what the module checked, printed once (the totals of a whole run are in the commit message)"""
    yield
    print(f"\nguarded allocations checked: {ga.CHECKED['allocations']} in {ga.CHECKED['arenas']} arenas, "
          f"{ga.CHECKED['bytes']} payload bytes")


@contextlib.contextmanager
def _nothing_after_a_gpu_fault(cid):
    """a HIP error ends the run: after a fault nothing more is started on the card"""
    try:
        yield
    except Exception as e:
        if any(s in f"{type(e).__name__} {e}" for s in ("HIP error", "hipError", "illegal memory access", "AcceleratorError")):
            pytest.exit(f"{cid}: the GPU reported {e!r}; no further test is started", returncode=3)
        raise


@pytest.mark.parametrize("cid", [c for c in gc.CASE_IDS if c not in END_TO_END])
def test_guards_hold_and_results_do_not_depend_on_the_fill(cid, monkeypatch):
    with _nothing_after_a_gpu_fault(cid):
        _guards_hold(cid, monkeypatch)


def _guards_hold(cid, monkeypatch):
    built = BUILDERS[cid]()
    fn, compare = built if isinstance(built, tuple) else (built, same_bits)
    assert (cid in gc.NOT_BIT_EXACT) == (compare is not same_bits), "exemptions are those of guarded_cases.NOT_BIT_EXACT"
    want = fn()
    torch.cuda.synchronize()
    got = ga.run_guarded(fn, monkeypatch=monkeypatch)          # (raises GuardCorrupted with the allocation's call site)
    counts = {fill: len(arena.allocations) for fill, arena in ga.run_guarded.arenas.items()}
    assert all(counts.values()) and len(set(counts.values())) == 1, f"allocations through the shim per fill: {counts}"
    print(f"{cid}: {counts[0x00]} guarded allocations per fill, "
          f"{sum(a.nbytes for a in ga.run_guarded.arenas[0xFF].allocations)} bytes")
    for fill, out in got.items():
        compare(want, out, f"{cid}, fill {fill:#04x} against the plain call")
    compare(got[0x00], got[0xFF], f"{cid}, fill 0x00 against fill 0xff")


# ---- inputs --------------------------------------------------------------------------------------------------------
def _index(seed, m, n_cells, mean, tomb=25, sizes=None, dup=0.0):
    """test_gpu_kernels._random_index at the first seed whose storage capacity is no multiple of 32"""
    from test_gpu_kernels import _random_index
    for s in range(seed, seed + 64):
        rng = np.random.default_rng(s)
        index = _random_index(rng, m, n_cells, mean, tomb, dup, sizes=sizes)
        if index[0].shape[1] % 32:
            return rng, index
    raise AssertionError("no seed gives a capacity that is no multiple of 32")


def _probes(rng, nq, n_cells, n_probe, start, sizes, ragged=True):
    """probe lists as test_scan_random_vs_oracle draws them: a cell listed twice in a row, per-query probe counts"""
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    if nq > 3 and n_probe > 1:
        cells[3, 1] = cells[3, 0]
    npl = rng.integers(0, n_probe + 1, nq).astype(np.int64) if ragged else np.full(nq, n_probe, np.int64)
    npl[:min(nq, 5)] = n_probe
    return cells, start[cells], sizes[cells], npl


def _ragged_sizes(n_cells, mean, tile):
    """test_scan_large_batch_routes_vs_oracle's cell sizes: unequal, one empty, none a multiple of the tile"""
    sizes = mean - 20 + (np.arange(n_cells) * 7) % 41
    sizes[sizes % tile == 0] += 1
    sizes[0] = 0
    return sizes


def _plain_scan(seed, m, nq, k, n_probe, n_cells=40, mean=150, tomb=25, ds=2, sizes=None, scale=100.0, lut=True):
    """a random index, its probes, a caller's table and (query, codebook) on the GPU"""
    rng, (storage, is_empty, start, sizes, a2i) = _index(seed, m, n_cells, mean, tomb, sizes)
    cells, cs, sz, npl = _probes(rng, nq, n_cells, n_probe, start, sizes)
    p = dict(m=m, nq=nq, k=k, n_probe=n_probe, ds=ds, n_slots=storage.shape[1], n_cells=n_cells, rng=rng,
             st=T(storage), emp=T(is_empty), a2i=T(a2i), cs=T(cs), sz=T(sz), npl=T(npl), cells=T(cells),
             start=T(start), sizes=T(sizes))
    if lut:
        p["lut"] = T((rng.standard_normal((m, nq, 256)) * scale).astype(np.float32))
    p["cb"] = T((rng.standard_normal((m, ds, 256)) * 20).astype(np.float32))
    p["q"] = T((rng.standard_normal((m * ds, nq)) * 20).astype(np.float32))
    return p


def _topk(scan, p, packed, n_split=None, hint=None, k=None):
    return scan.topk(p["st"], p["lut"], p["emp"], p["cs"], p["sz"], p["npl"], n_candidates=k or p["k"], packed=packed,
                     address2id=p["a2i"], n_split=n_split, slots_hint=hint)


def _fused(scan, p, packed, n_split=None, hint=None, **kw):
    return scan.topk_fused(p["st"], p["q"], p["cb"], p["emp"], p["cs"], p["sz"], p["npl"], p["k"], packed=packed,
                           address2id=p["a2i"], n_split=n_split, slots_hint=hint, **kw)


# ---- IVFPQTopkHip, plain ----------------------------------------------------------------------------------------------
@case("scan_reference_layout_m8")
def _():
    K, p = kernels(), _plain_scan(801, 8, 37, 10, 6, ds=4)

    def fn():
        scan, out = K.IVFPQTopkHip(m=8), []
        for n_split in (1, 3):
            out.append(_topk(scan, p, None, n_split))
            assert scan.last_route() == "reference_layout" and scan.last_n_split == n_split
            out.append(_fused(scan, p, None, n_split))
            assert scan.last_route() == "reference_layout"
        return out
    return fn


@case("scan_one_launch_m16_split7_tickets")
def _():
    K, p = kernels(), _plain_scan(1601, 16, 37, 10, 8)

    def fn():
        scan = K.IVFPQTopkHip(m=16)          # (a fresh wrapper: its ticket buffer is this run's own zeroed allocation)
        packed = K.PackCodesHip()(p["st"])
        a = _topk(scan, p, packed, 7)
        assert scan.last_route() == "one_launch_finish"
        b = _fused(scan, p, packed, 7)
        assert scan.last_route() == "one_launch_finish" and len(scan._ticket_cache) == 1
        tickets = next(iter(scan._ticket_cache.values()))
        return a, b, tickets.clone()                      # every call leaves its tickets zero
    return fn


@case("scan_three_launch_direct_no_tickets")
def _():
    """tpq_ivfpq_scan_topk_packed / tpq_ivfpq_search_fused -- the entry points without tickets, which no wrapper
    reaches: a split query then takes the sorted lists and the merge kernel"""
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    K, p, lib = kernels(), _plain_scan(1602, 16, 37, 10, 8), load()
    m, nq, k, n_probe, ds, n_split = 16, 37, 10, 8, 2, 3
    for has_lut in (1, 0):
        assert lib.tpq_ivfpq_scan_route(nq, k, n_split, m, ds, n_probe, 0, has_lut, 1, 0, 0) == 2   # sorted_lists

    def fn():
        packed = K.PackCodesHip()(p["st"])
        ws_bytes = lib.tpq_ivfpq_scan_workspace_bytes(nq, k, n_split, m)
        out = []
        for fused in (False, True):
            v, a, ids = gempty(nq, k, dtype=F32), gempty(nq, k, dtype=I64), gempty(nq, k, dtype=I64)
            ws = gempty(ws_bytes, dtype=U8)
            tail = (ptr(p["emp"]), ptr(p["cs"]), ptr(p["sz"]), ptr(p["npl"]), ptr(v), ptr(a), ptr(p["a2i"]), ptr(ids),
                    p["n_slots"], nq, n_probe, m, k, n_split, ptr(ws), ws_bytes, stream_ptr(DEV))
            with torch.cuda.device(DEV):
                if fused:
                    rc = lib.tpq_ivfpq_search_fused(ptr(packed), ptr(p["st"]), ptr(p["q"]), ptr(p["cb"]), ds, 0, *tail)
                else:
                    rc = lib.tpq_ivfpq_scan_topk_packed(ptr(packed), ptr(p["st"]), ptr(p["lut"]), *tail)
            check(rc, "direct scan call")
            out.append((v, a, ids))
        return out
    return fn


@case("scan_pools_m64_k600")
def _():
    K, p = kernels(), _plain_scan(6401, 64, 9, 600, 20, n_cells=48, mean=330, tomb=40)

    def fn():
        scan = K.IVFPQTopkHip(m=64)
        out = _topk(scan, p, K.PackCodesHip()(p["st"]), 2)
        assert scan.last_route() == "pools"
        return out
    return fn


def _pool_max_split(m, k):
    """csrc/scan_host.h pool_max_split: splits per query the ranking kernel's 64 KiB of LDS can take"""
    nw = 4 if m <= 32 else (8 if m <= 64 else 16)
    length = 64 * (8 if nw == 4 else 4)
    return max(1, (65536 - (k + 63) // 64 * 64 * 8) // (nw * length * 8))


@case("scan_pools_split_clamp_m120_k1000")
def _():
    K, p = kernels(), _plain_scan(12001, 120, 7, 1000, 20, n_cells=48, mean=330, tomb=40)
    n_split = 3
    assert _pool_max_split(120, 1000) == 1 < n_split and _pool_max_split(64, 600) == 3   # the library clamps this call

    def fn():
        scan = K.IVFPQTopkHip(m=120)
        out = _topk(scan, p, K.PackCodesHip()(p["st"]), n_split)
        assert scan.last_route() == "pools"
        return out
    return fn


@case("scan_dump_f32_m16_k40")
def _():
    K = kernels()
    mean, n_probe = 300, 8
    p = _plain_scan(1603, 16, 1024, 40, n_probe, mean=mean, tomb=0, sizes=_ragged_sizes(40, mean, 256), lut=False)
    p["lut"] = K.AdcLutHip()(p["q"], p["cb"])

    def fn():
        scan = K.IVFPQTopkHip(m=16)
        packed = K.PackCodesHip()(p["st"])
        a = _fused(scan, p, packed, 1, n_probe * mean)
        assert scan.last_route() == "dump_f32"
        b = _topk(scan, p, packed, 1, 32 * 977)            # (a caller's table rides the route behind long scans only)
        assert scan.last_route() == "dump_f32"
        return a, b
    return fn


def _sel16_batch(seed, nq, k, n_probe, mean, tomb=25):
    p = _plain_scan(seed, 64, nq, k, n_probe, mean=mean, tomb=tomb, sizes=_ragged_sizes(40, mean, 64), lut=False)
    p["hint"] = n_probe * mean
    return p


def _slots():
    return 4 * torch.cuda.get_device_properties(0).multi_processor_count   # four dump-mode workgroups per CU


@case("scan_dump_sel16_split_tail_ordered")
def _():
    K, p = kernels(), _sel16_batch(6402, 1250, 100, 5, 150)
    assert _slots() < p["nq"] < 2 * _slots(), "the batch is one round of workgroup slots and a tail"

    def fn():
        scan = K.IVFPQTopkHip(m=64)
        out = _fused(scan, p, K.PackCodesHip()(p["st"]), 1, p["hint"])
        assert scan.last_route() == "dump_sel16" and scan.last_ordered() is True and scan.last_cell_major() is False
        return out
    return fn


@case("scan_dump_sel16_lists_in_use_only")
def _():
    """the wrapper's workspace_bytes set to what the lists in use take and not a byte more -- less than the rule before
    the split tail sized it: the tail stays whole, the order is off, and the canary sits right behind the last list"""
    from test_gpu_scan_order import _lists_in_use
    K, p = kernels(), _sel16_batch(6402, 1250, 100, 5, 150)
    probe = K.IVFPQTopkHip(m=64)
    packed = K.PackCodesHip()(p["st"])
    _fused(probe, p, packed, 1, p["hint"])
    exact = _lists_in_use(probe)
    assert exact < probe.last_workspace_bytes

    def fn():
        scan = K.IVFPQTopkHip(m=64)
        scan.workspace_bytes = exact
        out = _fused(scan, p, packed, 1, p["hint"])
        assert scan.last_route() == "dump_sel16" and scan.last_ordered() is False and scan.last_workspace_bytes == exact
        return out
    return fn


@case("scan_dump_sel16_w8_k300")
def _():
    K, p = kernels(), _sel16_batch(6403, 1024, 300, 4, 450, tomb=0)

    def fn():
        scan = K.IVFPQTopkHip(m=64)
        out = _fused(scan, p, K.PackCodesHip()(p["st"]), 1, p["hint"])
        assert scan.last_route() == "dump_sel16_w8"
        return out
    return fn


def _cell_major(norms):
    from test_gpu_scan_cell_norms import _align
    from test_gpu_scan_cells import P0, _problem
    from torchpq_amd import _lib
    K = kernels()
    nq, n_cells, n_probe, k = 1024, 8, P0 + 1, 100          # the smallest probe count the form takes
    p = _problem(nq + n_cells + n_probe + k, nq, n_cells, n_probe, 2)
    assert p["n_slots"] % 32 != 0
    cs, sz = p["start"][p["cells"]].contiguous(), p["sizes"][p["cells"]].contiguous()
    hint = int(p["sizes"].float().mean().item() * n_probe)
    packed = K.PackCodesHip()(p["storage"])
    lists16 = 2 * _align(nq * 4) + nq * 16 * 64 * 8 + _align(nq * 16 * 4)
    no_room = lists16 + _lib.load().tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, n_cells, P0)

    def fn():
        scan = K.IVFPQTopkHip(m=64)
        scan.workspace_bytes = None if norms else no_room
        out = scan.topk_fused(p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], k, packed=packed,
                              slots_hint=hint, cells=p["cells"], n_cells=n_cells)
        assert scan.last_route() == "dump_sel16" and scan.last_cell_major() is True
        assert scan.last_cell_norms() is norms
        return out
    return fn


case("scan_cell_major_slot_norms")(lambda: _cell_major(True))
case("scan_cell_major_own_norms")(lambda: _cell_major(False))


@case("scan_exact_redo_in_a_dump_batch")
def _():
    """test_tables_the_16_bit_scale_cannot_hold_go_to_the_exact_kernel's queries in a batch with a split tail: one at
    1e19 (|q|^2 overflows), one component at 3e18, one all zero -- flagged by the scan, redone by the exact kernel"""
    K, p = kernels(), _sel16_batch(6404, 1100, 50, 8, 190)
    q = p["q"].clone()
    q[:, 3] = 1e19
    q[5, 1000] = 3e18
    q[:, 1099] = 0.0
    p["q"] = q

    def fn():
        scan = K.IVFPQTopkHip(m=64)
        scan.keep_workspace = True
        out = _fused(scan, p, K.PackCodesHip()(p["st"]), 1, p["hint"])
        assert scan.last_route() == "dump_sel16"
        redone = scan.last_redone(p["nq"])
        assert redone >= 1                 # (the query at 1e19 for sure)
        return out, redone
    return fn


@case("scan_exact_redo_in_one_launch")
def _():
    """test_scan_short_lists_overflow_is_redone_exactly at m = 16, k = 100: all of query 0's best vectors in tiles of
    wave 0 -- its short list overflows, the finisher's own redo branch takes the query"""
    K = kernels()
    m, k, n, nq = 16, 100, 32768, 3
    rng = np.random.default_rng(m * 1000 + k)
    lut = (rng.standard_normal((m, nq, 256)) * 100).astype(np.float32)
    codes = rng.integers(0, 256, (n, m), dtype=np.uint8)
    top = np.nonzero((np.arange(n) // 64) % 32 == 0)[0]
    codes[top] = lut[:, 0, :].argmax(axis=1).astype(np.uint8)
    for t in top:
        codes[t, rng.choice(m, 2, replace=False)] = rng.integers(0, 256, 2)
    st = T(np.ascontiguousarray(codes.reshape(n, m // 4, 4).transpose(1, 0, 2)))
    lut, emp = T(lut), T(np.zeros(n, np.uint8))
    cs, sz, npl = T(np.zeros((nq, 1), np.int64)), T(np.full((nq, 1), n, np.int64)), T(np.ones(nq, np.int64))

    def fn():
        scan = K.IVFPQTopkHip(m=m)
        scan.keep_workspace = True
        out = scan.topk(st, lut, emp, cs, sz, npl, n_candidates=k, packed=K.PackCodesHip()(st), n_split=1, slots_hint=n)
        assert scan.last_route() == "one_launch_finish"
        redone = scan.last_redone(nq)
        assert redone >= 1
        return out, redone
    return fn


@case("scan_lds_fallback_m128")
def _():
    """test_scan_packed_falls_back_when_lds_is_short: a 700-entry probe table does not fit next to the 128-KiB table"""
    K = kernels()
    m, n_cells, nq, n_probe, k = 128, 800, 5, 700, 40
    rng, (storage, is_empty, start, sizes, a2i) = _index(77, m, n_cells, 6, 0)
    lut = T((rng.standard_normal((m, nq, 256)) * 100).astype(np.float32))
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    st, emp, cs, sz = T(storage), T(is_empty), T(start[cells]), T(sizes[cells])
    npl = T(np.full(nq, n_probe, np.int64))

    def fn():
        scan = K.IVFPQTopkHip(m=m)
        out = scan.topk(st, lut, emp, cs, sz, npl, n_candidates=k, packed=K.PackCodesHip()(st), n_split=2)
        assert scan.last_route() == "reference_layout"
        return out
    return fn


# ---- IVFPQTopkHip, residual -------------------------------------------------------------------------------------------
def _residual_inputs(seed, m, nq, n_probe, tomb, ds=2, n_cells=30):
    """test_residual_packed_scan_vs_oracle's inputs"""
    rng, (storage, is_empty, start, sizes, a2i) = _index(seed, m, n_cells, 140, tomb, dup=0.1)
    cells, cs, sz, npl = _probes(rng, nq, n_cells, n_probe, start, sizes)
    return dict(st=T(storage), emp=T(is_empty), a2i=T(a2i), start=T(start), sizes=T(sizes), cells=T(cells), cs=T(cs),
                sz=T(sz), npl=T(npl), part2=T((rng.standard_normal((n_cells, m, 256)) * 50).astype(np.float32)),
                cb=T((rng.standard_normal((m, ds, 256)) * 8).astype(np.float32)),
                q=T((rng.standard_normal((m * ds, nq)) * 8).astype(np.float32)),
                base=T((rng.standard_normal((nq, n_probe)) * 300).astype(np.float32)))


def _residual_sorted_lists(m, k, n_probe, tomb):
    K, r = kernels(), _residual_inputs(m * 11 + k, m, 21, n_probe, tomb)

    def fn():
        scan = K.IVFPQTopkHip(m=m)
        packed = K.PackCodesHip()(r["st"])
        slot_term, cell_bound = K.ResidualSlotTermsHip()(r["st"], r["part2"], r["start"], r["sizes"])
        part1 = K.ResidualPart1Hip()(r["q"], r["cb"])
        out = [slot_term, cell_bound, part1]
        for n_split in (1, 3):
            for given in (True, False):     # part1 given, or built in the workgroup from (query, codebook)
                out.append(scan.topk_residual_packed(
                    r["st"], packed, r["part2"], slot_term, cell_bound, r["cells"], r["base"], r["emp"], r["cs"], r["sz"],
                    r["npl"], n_candidates=k, part1=part1 if given else None, query=None if given else r["q"],
                    codebook=None if given else r["cb"], address2id=r["a2i"], n_split=n_split))
                assert scan.last_route() == "sorted_lists" and scan.last_n_split == n_split
        same_bits(out[3], out[4], "part1 given against part1 built")
        return out
    return fn


case("scan_residual_sorted_lists_m8")(lambda: _residual_sorted_lists(8, 10, 5, 0))
case("scan_residual_sorted_lists_m64")(lambda: _residual_sorted_lists(64, 100, 12, 30))


@case("scan_residual_full_table_and_precomputed")
def _():
    K, r = kernels(), _residual_inputs(66, 8, 21, 5, 5)
    part1 = K.ResidualPart1Hip()(r["q"], r["cb"])
    full = (part1[:, None] + r["part2"][r["cells"]]).contiguous()          # one table per (query, probe)

    def fn():
        scan = K.IVFPQTopkHip(m=8)
        a = scan.topk_residual_precomputed(r["st"], part1, r["part2"], r["cells"], r["base"], r["emp"], r["cs"], r["sz"],
                                           r["npl"], n_candidates=10, address2id=r["a2i"])
        b = scan.topk_residual(r["st"], full, r["base"], r["emp"], r["cs"], r["sz"], r["npl"], n_candidates=10)
        return a, b
    return fn


# ---- the other scan-side entry points ------------------------------------------------------------------------------
@case("adc_lut")
def _():
    K = kernels()
    rng = np.random.default_rng(804)
    cb, q = T((rng.standard_normal((8, 4, 256)) * 30).astype(np.float32)), T((rng.standard_normal((32, 37)) * 30).astype(np.float32))
    return lambda: [K.AdcLutHip()(q, cb, distance) for distance in ("euclidean", "cosine")]


@case("residual_part1")
def _():
    K = kernels()
    rng = np.random.default_rng(805)
    cb, q = T(rng.standard_normal((12, 3, 256)).astype(np.float32)), T(rng.standard_normal((36, 37)).astype(np.float32))
    return lambda: K.ResidualPart1Hip()(q, cb)


@case("residual_slot_terms")
def _():
    K, r = kernels(), _residual_inputs(806, 24, 5, 4, 9)
    return lambda: K.ResidualSlotTermsHip()(r["st"], r["part2"], r["start"], r["sizes"])


@case("scan_order")
def _():
    from test_gpu_scan_order import _order_inputs
    K = kernels()
    inputs = [([T(x) for x in _order_inputs(np.random.default_rng(nq * 100 + mp + shift), nq, mp, equal=False)], shift)
              for nq, mp, shift in ((1025, 8, 6), (63, 70, 8))]
    return lambda: [K.ScanOrderHip()(*args, shift) for args, shift in inputs]


def _cell_candidates(slot_norms):
    from test_gpu_scan_cell_norms import A_CAPACITY, _layout_a, _pairs, _run
    L = _layout_a(2)
    nq = L["nq"]

    def fn():
        return [_run(L, np.full(nq, -np.inf), metric, first, A_CAPACITY, slot_norms)
                for metric, first in (("euclidean", 0), ("inner", 2))]

    def compare(a, b, where="result"):
        for run, (x, y) in enumerate(zip(a, b)):
            for name, i in (("count", 0), ("band", 3), ("flags", 4)):
                same_bits(x[i], y[i], f"{where}, call {run}, {name}")
            for qi, ((xa, xv), (ya, yv)) in enumerate(zip(_pairs(L, x, A_CAPACITY), _pairs(L, y, A_CAPACITY))):
                assert np.array_equal(xa, ya) and np.array_equal(xv, yv), (where, run, qi)
    return fn, compare


case("cell_candidates_slot_norms")(lambda: _cell_candidates(True))
case("cell_candidates_own_norms")(lambda: _cell_candidates(False))


@case("slot_filter_build_77")
def _():
    K = kernels()
    n_slots = 77
    rng = np.random.default_rng(n_slots)
    adr = T(np.concatenate([rng.integers(0, n_slots, 40), [-1, n_slots, n_slots + 31, -(1 << 40), 1 << 40, n_slots - 1]])
            .astype(np.int64))

    def fn():
        bits = gempty((n_slots + 31) // 32, dtype=I32)       # exactly ceil(n_slots / 32) words: the last one is partial
        bits.zero_()
        assert K.SlotFilterBuildHip()(adr, bits, n_slots) is bits
        return bits
    return fn


# ---- filtered search ---------------------------------------------------------------------------------------------------
def _filtered_plain(m, ds):
    import ivfpq_filtered_cases as fcases
    from test_gpu_ivfpq_filtered import _gpu, _run_plain
    from torchpq_amd.kernels import IVFPQFilteredTopkHip
    c = fcases.plain_case(m, ds, "fused", 3, 8, "euclidean")
    assert c["storage"].shape[1] % 32 != 0
    _gpu(c)

    def fn():
        op, out = IVFPQFilteredTopkHip(m=m), []
        for n_split in (1, 5):
            for run, k in ((0, 10), (1, 100), (len(c["runs"]) - 1, 10)):      # (the last run passes no row per query)
                out.append(_run_plain(c, "fused", "euclidean", run, k, n_split, op))
                assert op.last_n_split == n_split
        return out
    return fn


case("filtered_plain_m8")(lambda: _filtered_plain(8, 4))
case("filtered_plain_m148")(lambda: _filtered_plain(148, 1))        # the largest m the kernel admits


def _filtered_residual(m, ds):
    import ivfpq_filtered_cases as fcases
    from test_gpu_ivfpq_filtered import _gpu, _run_residual
    c = fcases.residual_case(m, ds, "part1", 3, 8)
    _gpu(c)
    return lambda: [_run_residual(c, tables, run, k) for tables in ("part1", "built") for run, k in ((0, 10), (1, 100))]


case("filtered_residual_m8")(lambda: _filtered_residual(8, 4))
case("filtered_residual_m148")(lambda: _filtered_residual(148, 1))


# ---- range search and the other list scans ------------------------------------------------------------------------
@case("ivfpq_range_plain")
def _():
    import ivfpq_range_cases as rcases
    from test_gpu_ivfpq_range import _run_plain
    from torchpq_amd.kernels import IVFPQRangeHip
    fused = rcases.plain_case(16, 4, "fused", 6, 8, "euclidean")
    table = rcases.plain_case(20, 8, "materialised", 3, 8, "euclidean")

    def fn():
        out = []
        for c, kind, m in ((fused, "fused", 16), (table, "materialised", 20)):
            op = IVFPQRangeHip(m=m)
            for n_split in (None, 1, 5):
                out.append(_run_plain(c, kind, "euclidean", c["runs"][0], n_split, op))
                assert op.last_n_split == n_split if n_split else op.last_n_split > 1
            out.append(_run_plain(c, kind, "euclidean", float("-inf"), 7, op))     # every candidate is a hit
        return out
    return fn


@case("ivfpq_range_residual")
def _():
    import ivfpq_range_cases as rcases
    from test_gpu_ivfpq_range import _run_residual
    cs = [(rcases.residual_case(m, ds, tables, 3, 8), tables) for m, ds, tables in
          ((8, 4, "part1"), (64, 2, "built"), (16, 8, "full"))]
    return lambda: [_run_residual(c, tables, thr) for c, tables in cs for thr in (c["runs"][0], float("-inf"))]


def _flat_lists():
    from test_gpu_ivfflat import _case
    c = _case(1000 * 24 + 5 + 8, 24, 5, 8)
    assert c["vectors"].shape[1] % 32 != 0
    return c


@case("ivfflat_topk")
def _():
    from test_gpu_ivfflat import _run
    c = _flat_lists()

    def fn():
        out = []
        for n_split in (None, 1, 6):
            v, a, op = _run(c, 100, "euclidean", n_split)
            assert op.last_n_split == n_split if n_split else op.last_n_split > 1
            out.append((v, a))
        return out
    return fn


@case("ivfflat_range")
def _():
    from test_gpu_ivfflat import _run as topk
    from test_gpu_ivfflat_range import _run
    c = _flat_lists()
    thr = np.ascontiguousarray(topk(c, 10, "euclidean", 1)[0][:, 9])       # the 10th best value (-inf: every candidate)

    def fn():
        out = []
        for n_split in (None, 1, 6):
            lims, v, a, op = _run(c, thr, "euclidean", n_split)
            assert op.last_n_split == n_split if n_split else op.last_n_split > 1
            out.append((lims, v, a))
        return out
    return fn


@case("ivfpq4_topk")
def _():
    import ivfpq4_cases as cases
    from test_gpu_ivfpq4 import _run
    c = cases.case(16013, 16, 2, 5, 8)
    assert c["storage"].shape[1] % 32 != 0

    def fn():
        out = []
        for n_split in (None, 1, 3):
            v, a, op = _run(c, 100, "euclidean", n_split)
            assert op.last_n_split == n_split if n_split else op.last_n_split > 1
            out.append((v, a))
        return out
    return fn


@case("ivfpq4_residual_topk")
def _():
    import ivfpq4_residual_cases as cases
    from test_gpu_ivfpq4_residual import _run
    c = cases.case(16013, 16, 2, 5, 8)

    def fn():
        out = []
        for n_split in (None, 1, 3):
            v, a, op = _run(c, 100, "euclidean", n_split)
            assert op.last_n_split == n_split if n_split else op.last_n_split > 1
            out.append((v, a))
        return out
    return fn


@case("ivfpqr_rerank")
def _():
    from tests_support import _case
    K = kernels()
    m, k = 8, 10
    storage, cb, cb_r, query, cand, a2i = (T(x) for x in _case(5, m, 16, 32, 333, 130, 16, "euclidean"))
    return lambda: [K.IVFPQRerankHip()(storage, m, cb if res else None, cb_r, query, cand, k, use_residual=res,
                                       distance="euclidean", address2id=a2i) for res in (True, False)]


def _flat_problem():
    from test_gpu_flat_range import _problem
    return _problem(17000 + 1000 + 130, 17, 1000, 130)           # four 256-slot chunks, the last of 232 slots


@case("flat_topk")
def _():
    K = kernels()
    y, x, a2id = (T(t) for t in _flat_problem())

    def fn():
        op, out = K.FlatTopkHip(), []
        # 3 parts of two chunks: the third holds nothing; 7 parts: more parts than chunks; 1: no merge of lists
        for n_parts in (3, 7, 1, None):
            out.append(op(y, x, 70, address2id=a2id, n_parts=n_parts))
            assert n_parts is None or op.last_n_parts == n_parts
        for other in out[1:]:
            same_bits(out[0], other, "the result does not depend on n_parts")
        return out
    return fn


@case("flat_range")
def _():
    import flat_range_oracle as frorc
    from test_gpu_flat_range import _run, _thresholds
    y, x, a2id = _flat_problem()
    thr = _thresholds(frorc.values(y, x, "euclidean"), a2id)
    return lambda: [_run(y, x, thr, a2id, "euclidean", n_parts) for n_parts in (None, 2, 7)]


# ---- the coarse step -------------------------------------------------------------------------------------------------
def _coarse_probe(d, nq, n_cells, n_probe, smart, fp16):
    """every route the shape admits, the fp16 route with a prepared block and with none; `fp16`: whether the shape has
    an fp16 selection pass at all (tpq_ivfpq_coarse_probe_prepared_bytes says so)"""
    from test_gpu_round3 import _probe_data
    from torchpq_amd import _lib
    K = kernels()
    assert (_lib.load().tpq_ivfpq_coarse_probe_prepared_bytes(d, n_cells) > 0) == fp16
    rng = np.random.default_rng(1000 * d + nq)
    x, c = _probe_data("gauss", d, nq, n_cells, rng)
    sizes = rng.integers(0, 500, n_cells).astype(np.int64)
    start = (np.cumsum(sizes + 3) - sizes - 3).astype(np.int64)
    x, c, start, sizes = T(x), T(c), T(start), T(sizes)

    def fn():
        out = {route: K.CoarseProbeHip(route=route)(x, c, start, sizes, n_probe, 30.0 if smart else None)
               for route in ("auto", "fp32", "fp16")}
        prepared = K.CoarseProbeHip.prepare(c)
        assert (prepared is not None) == fp16
        if fp16:
            out["fp16, prepared"] = K.CoarseProbeHip(route="fp16")(x, c, start, sizes, n_probe, 30.0 if smart else None,
                                                                   prepared=prepared)
        for route in ("auto", "fp16") + (("fp16, prepared",) if fp16 else ()):
            same_bits(out["fp32"], out[route], f"route {route} against fp32")
        return out
    return fn


case("coarse_probe_d32_nq5_all_cells")(lambda: _coarse_probe(32, 5, 16, 16, False, False))
case("coarse_probe_d7_one_query_one_probe")(lambda: _coarse_probe(7, 1, 40, 1, True, False))
case("coarse_probe_fp16_last_group_half_full")(lambda: _coarse_probe(64, 500, 12320, 24, True, True))
case("coarse_probe_group_filter")(lambda: _coarse_probe(8, 1100, 16500, 100, True, False))
case("coarse_probe_600_probes")(lambda: _coarse_probe(16, 3, 1024, 600, True, True))


@case("coarse_probe_direct_auto")
def _():
    """tpq_ivfpq_coarse_probe, the entry point without a route argument, which no wrapper reaches"""
    from test_gpu_round3 import _probe_data
    from torchpq_amd._lib import check, load, ptr, stream_ptr
    lib = load()
    d, nq, n_cells, n_probe = 32, 77, 300, 9
    rng = np.random.default_rng(1000 * d + nq)
    x, c = _probe_data("gauss", d, nq, n_cells, rng)
    sizes = rng.integers(0, 500, n_cells).astype(np.int64)
    x, c, start, sizes = T(x), T(c), T((np.cumsum(sizes + 3) - sizes - 3).astype(np.int64)), T(sizes)

    def fn():
        ws_bytes = lib.tpq_ivfpq_coarse_probe_workspace_bytes(nq, n_cells)
        out = [gempty(nq, n_probe, dtype=F32)] + [gempty(nq, n_probe, dtype=I64) for _ in range(3)] + [gempty(nq, dtype=I64)]
        ws = gempty(max(ws_bytes, 1), dtype=U8)
        with torch.cuda.device(DEV):
            rc = lib.tpq_ivfpq_coarse_probe(ptr(x), ptr(c), ptr(start), ptr(sizes), *(ptr(t) for t in out), d, nq,
                                            n_cells, n_probe, 30.0, ptr(ws), ws_bytes, stream_ptr(DEV))
        check(rc, "tpq_ivfpq_coarse_probe")
        return out
    return fn


@case("topk_select")
def _():
    K = kernels()
    xs = []
    for rows, cols, k in ((3, 70, 70), (2, 5000, 1024)):
        x = np.random.default_rng(rows * cols + k).standard_normal((rows, cols)).astype(np.float32)
        x[:, ::3] = np.round(x[:, ::3], 1)                                   # plenty of exact ties
        xs.append((T(x), k))
    return lambda: [K.TopkSelectHip()(x, k=k) for x, k in xs]


@case("coarse_select")
def _():
    K = kernels()
    rng = np.random.default_rng(807)
    x, c = T((rng.standard_normal((32, 77)) * 30).astype(np.float32)), T((rng.standard_normal((32, 300)) * 30).astype(np.float32))
    dots, a2, b2 = (x.transpose(0, 1).contiguous() @ c).contiguous(), (x * x).sum(0), (c * c).sum(0)
    return lambda: [K.CoarseSelectHip()(dots, a2, b2, k) for k in (1, 33, 300)]


@case("smart_probing")
def _():
    K = kernels()
    s = -np.abs(np.random.default_rng(808).standard_normal((77, 33)).astype(np.float32)) * 5e4
    s = T(-np.sort(-s, axis=1))
    return lambda: K.SmartProbingHip()(s, 30.0)


# ---- k-means and assign -------------------------------------------------------------------------------------------------
def _max_sim(shape, precision, split):
    K = kernels()
    l, d, m, n = shape
    rng = np.random.default_rng(l * 1000 + d * 10 + n)
    A = (rng.standard_normal((l, d, m)) * 10).astype(np.float32)
    B = (A[:, :, rng.integers(0, m, n)] + rng.standard_normal((l, d, n))).astype(np.float32)
    B[:, :, n // 2] = B[:, :, 0]                                              # an exact tie: the smaller index wins
    A, B = T(A), T(B)
    if precision == "bf16x3":          # which kernel the wrapper calls: the split one, or tpq_max_sim in its place
        assert K.MaxSimHip.split_supported(d, m, n) == split

    def fn():
        return [K.MaxSimHip(distance=distance, precision=precision)(A, B, dim=2, mode="tn")
                for distance in ("euclidean", "inner")]
    return fn


case("max_sim_fp32")(lambda: _max_sim((2, 8, 257, 256), "fp32", False))
case("max_sim_bf16x3")(lambda: _max_sim((1, 17, 1000, 200), "bf16x3", True))
case("max_sim_bf16x3_unsupported_shape")(lambda: _max_sim((1, 65, 100, 7), "bf16x3", False))   # -> the fp32 kernel


def _coarse_assign(A, B, route, rechecked):
    """`rechecked`: what last_rechecked() must say of the route taken, as a predicate of (count, m)"""
    K = kernels()
    A, B = T(A), T(B)
    d, m = A.shape
    assert K.CoarseAssignHip.supported(d, m, B.shape[1])

    def fn():
        op = K.CoarseAssignHip(distance="euclidean", route=route)
        vals, labels = op(A, B, return_vals=True)
        count = op.last_rechecked()
        assert rechecked(count, m), (count, m)
        return vals, labels, count, op(A, B)                       # (and without the maxima: a null output pointer)
    return fn


@case("coarse_assign_auto")
def _():
    rng = np.random.default_rng(2)
    x = rng.standard_normal((960, 300)).astype(np.float32)
    return _coarse_assign(x, x[:, :70].copy(), None, lambda c, m: c == 0)          # small: tpq_max_sim inside


@case("coarse_assign_cascade_narrow")
def _():
    """test_centroids_beyond_the_fp16_range_of_the_data_scale_go_exact at (64, 5644, 1905): the chunked candidate route,
    every point listed and sent to the exact kernel"""
    d, m, n = 64, 5644, 1905
    rng = np.random.default_rng(d + m)
    x = (1000.0 + rng.standard_normal((d, m))).astype(np.float32)
    cent = (x[:, rng.integers(0, m, n)] + 50.0 * rng.standard_normal((d, n))).astype(np.float32)
    return _coarse_assign(x, cent, "cascade", lambda c, m: c == m)


def _wide(d, m, n):
    from test_gpu_lloyd import _data
    x, cent = _data("gauss", 1, d, m, n, np.random.default_rng(hash((d, m, n)) % 2 ** 31))
    return _coarse_assign(x[0], cent[0], "cascade", lambda c, m: 0 <= c <= m)


case("coarse_assign_cascade_wide")(lambda: _wide(129, 1000, 300))
case("coarse_assign_cascade_wide_one_centroid")(lambda: _wide(300, 260, 1))


@case("coarse_assign_candidate_overflow")
def _():
    """test_wide_assign_ties_overflow_and_flags: 2 000 identical centroids -- every centroid a candidate of every point,
    the pair list overflows and the exact kernel takes over"""
    x = np.random.default_rng(5).integers(-9, 9, (160, 3000)).astype(np.float32)
    fn = _coarse_assign(x, np.repeat(x[:, :1], 2000, axis=1), "cascade", lambda c, m: c == m)

    def checked():
        out = fn()
        assert int(out[1].abs().max().item()) == 0
        return out
    return checked


@case("coarse_assign_direct")
def _():
    """tpq_coarse_assign, the entry point without a route argument, which no wrapper reaches"""
    from torchpq_amd._lib import METRIC_NEG_SQ_L2, check, load, ptr, stream_ptr
    lib = load()
    d, m, n = 64, 801, 400
    rng = np.random.default_rng(809)
    A = T((rng.standard_normal((d, m)) * 10).astype(np.float32))
    B = T((rng.standard_normal((d, n)) * 10).astype(np.float32))

    def fn():
        ws_bytes = lib.tpq_coarse_assign_workspace_bytes(d, m, n)
        vals, labels, ws = gempty(m, dtype=F32), gempty(m, dtype=I64), gempty(max(ws_bytes, 1), dtype=U8)
        with torch.cuda.device(DEV):
            rc = lib.tpq_coarse_assign(ptr(A), ptr(B), ptr(vals), ptr(labels), d, m, n, METRIC_NEG_SQ_L2, ptr(ws),
                                       ws_bytes, stream_ptr(DEV))
        check(rc, "tpq_coarse_assign")
        off = lib.tpq_coarse_assign_count_offset(d, m, n)
        return vals, labels, ws[off:off + 4].view(I32).clone()
    return fn


@case("max_sim_select_cached_workspace")
def _():
    from test_gpu_kernels import _coarse_case
    K = kernels()
    rng = np.random.default_rng(2 * 100 + 40 * 7 + 200)
    As, Bs = zip(*[_coarse_case(rng, 40, 2500, 200, "sift") for _ in range(2)])
    A, B = T(np.stack(As)), T(np.stack(Bs))
    A_short = A[:, :, :1001].contiguous()
    assert K.MaxSimSelectHip.supported(2, 40, 2500, 200)

    def fn():
        op = K.MaxSimSelectHip(distance="euclidean")
        first = op(A, B)
        ws = op._ws
        second = op(A_short, B)                  # fewer points: the cached workspace of the first call serves again
        third = op(A, B)
        assert op._ws is ws
        same_bits(first, third, "the same call on a workspace two calls have used")
        return first, second
    return fn


@case("lloyd_prepare_and_two_steps")
def _():
    from test_gpu_lloyd import _data
    from test_gpu_lloyd_update import lloyd_bound
    K = kernels()
    l, d, n, k = 2, 40, 3001, 200
    x, cent = _data("gauss", l, d, n, k, np.random.default_rng(810))
    cent2 = (cent * np.float32(1.01)).astype(np.float32)
    X, C, C2 = T(x), T(cent), T(cent2)

    def fn():
        step = K.LloydStepHip(X, C)                  # prepare
        vals, labels, new = step(C, update=True)
        vals2, labels2, none = step(C2, update=False)
        assert none is None
        return dict(vals=vals, labels=labels, new=new, vals2=vals2, labels2=labels2, rechecked=step.rechecked())

    def compare(a, b, where="result"):
        for key in ("vals", "labels", "vals2", "labels2", "rechecked"):
            same_bits(a[key], b[key], f"{where}, {key}")
        for r in (a, b):
            lab, new = r["labels"].cpu().numpy(), r["new"].cpu().numpy()
            mean, bnd = lloyd_bound(x, cent, lab, k)
            assert np.isfinite(new).all() and (new[bnd == 0] == 0).all(), where
            assert (np.abs(new.astype(np.float64) - mean) <= bnd).all(), where
    return fn, compare


def _compute_centroids(shape, route):
    import centroid_oracle as O
    from test_gpu_centroid_update import _check_general
    K = kernels()
    l, d, n, k = shape
    assert O.route(*shape) == route
    rng = np.random.default_rng(O.seed(shape, "guarded"))
    lab = O.make_labels("uniform", l, n, k, rng, out_of_range=True)
    x = O.make_general("gauss", l, d, n, rng)
    xi, labi, expected = O.make_integers_small(lab, l, d, n, k, rng)
    X, L, Xi, Li = T(x), T(lab), T(xi), T(labi)

    def fn():
        op = K.ComputeCentroidsHip()
        return op(X, L, k=k), op(Xi, Li, k=k)

    def compare(a, b, where="result"):
        _check_general([a[0].cpu().numpy(), b[0].cpu().numpy()], x, lab, k, shape, "gauss", where)
        same_bits(a[1], b[1], f"{where}, small integers (exact in any order)")
        assert np.array_equal(b[1].cpu().numpy().view(np.uint32), expected.view(np.uint32)), where
    return fn, compare


case("compute_centroids_mfma")(lambda: _compute_centroids((1, 33, 8193, 255), "mfma"))        # two blocks per tile
case("compute_centroids_lds")(lambda: _compute_centroids((3, 31, 8196, 257), "lds"))
case("compute_centroids_lds_k2409")(lambda: _compute_centroids((1, 17, 4097, 2409), "lds"))   # the last k that fits
case("compute_centroids_global_k2410")(lambda: _compute_centroids((1, 16, 255, 2410), "global"))


# ---- containers -----------------------------------------------------------------------------------------------------------
@case("get_ioa")
def _():
    K = kernels()
    rng = np.random.default_rng(3)
    # (n_cells=None: the sort runs over all 31 key bits)
    inputs = [(T(rng.integers(0, top, n).astype(np.int64)), n_cells)
              for n, top, n_cells in ((1000, 5, 5), (4097, 16384, 16384), (257, 2 ** 31 - 2, None))]
    return lambda: [K.GetIOAHip()(labels, n_cells=n_cells) for labels, n_cells in inputs]


@case("get_write_address")
def _():
    from test_gpu_container_kernels import WA_CAP, WA_START, _wa_is_empty, _wa_queries
    K = kernels()
    is_empty = _wa_is_empty("random")[:-37]                     # the last cell: 263 of its 300 slots exist
    cells, ranks = _wa_queries(is_empty, seed=1)
    args = [T(x) for x in (is_empty, WA_START, WA_CAP, cells, ranks)]
    return lambda: K.GetWriteAddressHip()(*args)


@case("get_cell_by_address")
def _():
    from test_gpu_container_kernels import CELL_LAYOUTS, _edge_addresses
    K = kernels()
    start, cap = CELL_LAYOUTS["many"]
    adr, start, end = T(_edge_addresses(start, cap, 257)), T(start), T(start + cap)
    return lambda: K.GetCellByAddressHip()(adr, start, end)


@case("get_id_by_address")
def _():
    K = kernels()
    rng = np.random.default_rng(14)
    a2i = rng.integers(-1, 2 ** 62, 257)
    probe = np.concatenate([[-2 ** 40, -1, 0, 2 ** 40, 256, 257, 258], rng.integers(-3, 260, 257 * 3 - 7)]).astype(np.int64)
    a2i, probe = T(a2i), T(rng.permutation(probe).reshape(3, 257))
    return lambda: K.GetIdByAddressHip()(a2i, probe)


@case("get_address_by_id")
def _():
    from test_gpu_container_kernels import _id_queries, _id_table
    K = kernels()
    a2i, repeated = _id_table(4097, 3, 4097)
    a2i, ids = T(a2i), T(_id_queries(a2i, repeated, 257, 257))
    return lambda: K.GetAddressByIdHip()(a2i, ids)


@case("grow_cells")
def _():
    from test_gpu_container_kernels import GROW_LAYOUTS
    K = kernels()
    g = 3
    rng = np.random.default_rng(g * 100 + 5)
    old_cap, new_cap = (np.array(x, np.int64) for x in GROW_LAYOUTS["mixed"])
    old_start, new_start = np.cumsum(old_cap) - old_cap, np.cumsum(new_cap) - new_cap
    old_slots, new_slots = int(old_cap.sum()), int(new_cap.sum())
    assert new_slots % 32 != 0
    storage = rng.integers(1, 256, (g, old_slots, 4), dtype=np.uint8)
    is_empty = (rng.random(old_slots) < 0.3).astype(np.uint8)
    a2i = np.where(is_empty == 1, -1, rng.permutation(old_slots * 3)[:old_slots] + 1).astype(np.int64)
    args = [T(x) for x in (storage, a2i, is_empty, old_start, old_cap, new_start, new_cap)]
    return lambda: K.GrowCellsHip()(*args, new_slots)          # (the three new buffers are the wrapper's allocations)


@case("scatter_codes")
def _():
    from test_gpu_container_kernels import PACK_SLOTS, _pack_case
    K = kernels()
    m, n = 24, 257
    rng = np.random.default_rng(m + 1)
    storage, _ = _pack_case(m)
    assert PACK_SLOTS % 32 != 0
    codes = T(rng.integers(0, 256, (m, n), dtype=np.uint8))
    adr = rng.permutation(PACK_SLOTS)[:n].astype(np.int64)
    adr[rng.permutation(n)[:40]] = np.resize(np.array([-1, -1, PACK_SLOTS, PACK_SLOTS + 4, -2 ** 40, 2 ** 40, -1]), 40)
    adr, storage = T(adr), T(storage)

    def fn():
        st = gempty(*storage.shape, dtype=U8)                   # the kernel's targets: between canaries too
        st.copy_(storage)
        pk = K.PackCodesHip()(st)
        K.ScatterCodesHip()(codes, adr, st, pk)
        return st, pk
    return fn


def _pack_codes(m):
    K = kernels()
    storage = T(np.random.default_rng(m).integers(0, 256, (m // 4, 300, 4), dtype=np.uint8))

    def fn():
        whole = K.PackCodesHip()(storage)
        part = gempty(*whole.shape, dtype=U8)
        part.fill_(0xEE)
        assert K.PackCodesHip()(storage, part, 5, 300) is part          # slots [5, 300): the array's last slot included
        return whole, part
    return fn


case("pack_codes_m24")(lambda: _pack_codes(24))
case("pack_codes_m120")(lambda: _pack_codes(120))


@case("pq_decode")
def _():
    K = kernels()
    rng = np.random.default_rng(4 * 255)
    cb, codes = T(rng.standard_normal((4, 7, 256)).astype(np.float32)), T(rng.integers(0, 256, (4, 255), dtype=np.uint8))
    return lambda: K.PQDecodeHip()(cb, codes)


# ---- the index end to end ------------------------------------------------------------------------------------------
def _index_end_to_end(residual):
    """IVFPQIndex at d = 32, m = 8, 16 cells, 6 000 vectors.  The index is trained once (the Lloyd update sums with
    atomics: two trainings need not agree to the bit); every run loads that state into a fresh index and then adds,
    searches, grows and removes on its own -- each of those calls with an arena of its own, checked when it returns"""
    from tests_support import _clustered
    from torchpq_amd.index import IVFPQIndex
    d, n, more, nq, k = 32, 6000, 900, 50, 10
    base, queries = _clustered(11 + residual, d, n + more, nq)
    make = lambda: IVFPQIndex(d, n_subvectors=8, n_cells=16, initial_size=16, device=DEV, pq_use_residual=residual)  # noqa: E731
    np.random.seed(11)
    torch.manual_seed(11)
    trained = make()
    trained.train(T(base[:, :n]))
    state = {key: v.detach().cpu().clone() for key, v in trained.state_dict().items() if v is not None}
    x0, x1, xq = T(base[:, :n]), T(base[:, n:]), T(queries)
    ids0 = torch.arange(n, device=DEV) * 3 + 7
    allowed = [ids0[::2].contiguous(), torch.cat([ids0[:500], 3 * torch.arange(n, n + more, device=DEV) + 7])]
    rows = (torch.arange(nq, device=DEV) % 2).to(I32)

    def run(guard):
        idx = make()
        idx.load_state_dict({key: v.clone() for key, v in state.items()})
        idx.n_probe = 6
        out = []
        with guard():
            idx.add(x0, ids=ids0)
        flt = idx.id_filter(allowed)
        for phase in range(2):
            with guard():
                v, i = idx.search(xq, k=k)
            thr = v[:, k // 2].contiguous()                      # per query: its own 6th best value
            with guard():
                r = idx.range_search(xq, thr)
            with guard():
                f = idx.search_filtered(xq, k, flt, rows)
            out.append((v, i, r, f))
            if phase == 0:
                capacity = idx._storage.shape[1]
                with guard():
                    idx.add(x1, ids=3 * torch.arange(n, n + more, device=DEV) + 7)      # grows the buffers
                assert idx._storage.shape[1] > capacity
                with guard():
                    idx.remove(ids=ids0[1::7].contiguous())
        assert not torch.equal(out[0][1], out[1][1])
        return out
    return run


@pytest.mark.parametrize("cid,residual", [("index_plain_end_to_end", False), ("index_residual_end_to_end", True)])
def test_the_index_drives_the_wrappers_inside_their_buffers(cid, residual, monkeypatch):
    with _nothing_after_a_gpu_fault(cid):
        _index_stays_inside(cid, monkeypatch)


def _index_stays_inside(cid, monkeypatch):
    run = BUILDERS[cid]()
    want = run(contextlib.nullcontext)
    torch.cuda.synchronize()
    got, calls = {}, {}
    for fill in (0x00, 0xFF):
        arenas = []

        @contextlib.contextmanager
        def guard():
            with ga.guarded(monkeypatch, fill) as arena:
                yield
            arenas.append(arena)
        got[fill] = run(guard)
        calls[fill] = [len(a.allocations) for a in arenas]
        assert all(calls[fill]), calls[fill]
    assert calls[0x00] == calls[0xFF]
    print(f"{cid}: {len(calls[0x00])} guarded calls, {sum(calls[0x00])} guarded allocations per fill")
    for fill, out in got.items():
        same_bits(want, out, f"{cid}, fill {fill:#04x} against the plain run")


case("index_plain_end_to_end")(lambda: _index_end_to_end(False))
case("index_residual_end_to_end")(lambda: _index_end_to_end(True))


# ---- the harness on the GPU -----------------------------------------------------------------------------------------
def test_a_write_past_a_guarded_tensor_is_reported_on_the_gpu(monkeypatch):
    """the negative control: under an installed arena a torch indexing op sets the byte right behind a wrapper's
    allocation, through the arena's own buffer -- no library kernel is involved, no address outside a live allocation
    is touched -- and check() names that tensor and no other"""
    from torchpq_amd.kernels import _common
    arena = ga.Arena(torch, 0xFF, "cuda")
    with monkeypatch.context() as mp:
        ga.install(mp, arena)
        vals, address = _common.alloc_pair(3, 5, DEV)
    assert _common.torch is torch and len(arena.allocations) == 2
    assert vals.is_cuda and vals.data_ptr() % 512 == 0 and bool((address == -1).all())
    torch.cuda.synchronize()
    assert arena.check() == 2
    victim = arena.allocations[0]
    victim.buffer[ga.GUARD + victim.nbytes] = 0
    with pytest.raises(ga.GuardCorrupted) as err:
        arena.check()
    msg = str(err.value)
    assert "(3, 5)" in msg and "torch.float32" in msg and "_common.py" in msg and "torch.int64" not in msg
    assert "first at payload offset 60, last at payload offset 60" in msg and "1 byte(s) past its end" in msg
    victim.buffer[ga.GUARD + victim.nbytes] = ga.GUARD_BYTE
    assert arena.check() == 2
