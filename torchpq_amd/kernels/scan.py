"""The list scans and what feeds them: IVFPQ top-k (plain, fused LUT, residual), the LUT and residual tables, the
IVFPQR re-rank, the IVFFlat scan and range search, the 4-bit IVFPQ4 scan, the IVFPQ range search."""
import torch

from .._lib import check, load, ptr, require_gpu, stream_ptr
from ._common import alloc_pair, alloc_topk, call, metric_code, topk_result, workgroups_per_query

# n_subvectors with an instantiated scan-layout kernel (= TPQ_PACKED_M_LIST in csrc/scan_device.h)
PACKED_M = (4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 96, 120, 128)


def packed_chunk_width(m):
    return 16 if m % 16 == 0 else (8 if m % 8 == 0 else 4)


class CellKeptState:
    """The kept state of the cell-major form (csrc/scan_cells.hip, `The kept state`; tpq_ivfpq_search_fused_cells_kept):
    a caller-owned device buffer with what the form derives from codes, codebook and tombstones alone.  `key` is the
    owner's description of what it was derived from; the call that finds `valid` False builds the state on its
    stream, and `ready` -- recorded behind that call -- orders the first use on every other stream.  `builds` counts."""

    def __init__(self, n_bytes, device, key=None):
        self.buf = torch.empty(n_bytes, device=device, dtype=torch.uint8)
        self.key = key
        self.valid = False
        self.builds = 0
        self.ready = None

    def before_use(self, device):
        """orders the current stream behind the build, every time: a wait on an event that has completed, or that the
        stream is behind already, costs nothing on the device (a capturing stream is not asked to wait: whoever captures
        has run the warm-up searches and joined their stream, GraphedSearch)"""
        if self.valid and not torch.cuda.is_current_stream_capturing():
            torch.cuda.current_stream(device).wait_event(self.ready)

    def after_build(self, device):
        stream = torch.cuda.current_stream(device)
        self.ready = torch.cuda.Event()
        self.ready.record(stream)
        self.valid = True
        self.builds += 1


class IVFPQTopkHip:
    """IVF list scan + top-k.  Mirrors IVFPQTopkCuda (kernels/IVFPQTopkCuda.py:9-142);
    ``tpb``/``stack_capacity``/``sm_size`` are accepted for signature compatibility and
    ignored (the workgroup shape is fixed by the gfx950 kernel)."""

    def __init__(self, m=8, k=256, tpb=256, n_cs=4, stack_capacity=2, sm_size=None):
        assert k == 256  # 8-bit PQ only (IVFPQTopkCuda.py:21)
        assert n_cs == 4
        assert m % n_cs == 0
        self.m = m
        self.k = k
        self.tpb = tpb
        self.n_cs = n_cs
        self.n_cus = None
        # measurement hook (bench.py): when a list, every call appends a (start, stop) pair of
        # timing events recorded on the launch stream around the scan kernel(s)
        self.record_events = None
        self.last_n_split = None
        # tickets of the one-launch finish of split queries (tpq_ivfpq_*_tickets): caller-owned int32 [n_query],
        # zero between calls.  One buffer per (device, stream) -- calls that share a buffer must be ordered;
        # `ticket_buffer` overrides it (GraphedSearch hands in the buffer its graph owns).
        self.ticket_buffer = None
        self._ticket_cache = {}
        self.keep_workspace = False   # diagnostics: keep the last call's workspace in `last_workspace`
        self.last_workspace = None
        self.last_call = None         # diagnostics: the arguments of the last topk / topk_fused call (`last_route()`)
        # diagnostics / tests: bytes of workspace to hand to the library instead of tpq_ivfpq_scan_workspace_bytes (a
        # caller that sizes its workspace by an older rule); `last_workspace_bytes`: what the last call handed over
        self.workspace_bytes = None
        self.last_workspace_bytes = None
        self._last_device = None
        self._last_cells = None       # (n_cells, n_slots) when the last call handed over its probed cells
        self._last_withheld = False   # the last call switched the cell-major form's threshold form off
        self.last_cell_kept = None    # "built" / "reused": what the last call did with a kept state; None: it used none
        self._last_products = None    # tpq_ivfpq_scan_last_cell_products right after the last call

    def _tickets(self, n_query, n_split, device):
        """zeroed int32 [>= n_query] for this (device, current stream), or None (unsplit queries need none;
        inside a stream capture only a buffer handed in through `ticket_buffer` may be used: a fresh one
        would be zeroed by a captured memset on every replay)"""
        if n_split <= 1:
            return None
        if self.ticket_buffer is not None:
            t = self.ticket_buffer
            assert t.dtype == torch.int32 and t.numel() >= n_query and t.device == torch.device(device)
            return t
        if torch.cuda.is_current_stream_capturing():
            return None
        dev = torch.device(device)
        key = (dev.index, torch.cuda.current_stream(dev).cuda_stream)
        t = self._ticket_cache.get(key)
        if t is None or t.numel() < n_query:
            if len(self._ticket_cache) >= 64:
                self._ticket_cache.clear()
            t = torch.zeros(max(n_query, 1024), device=dev, dtype=torch.int32)
            self._ticket_cache[key] = t
        return t

    def _drop_tickets(self, device):
        """after a failed call the tickets may be left non-zero: never reuse them"""
        dev = torch.device(device)
        self._ticket_cache.pop((dev.index, torch.cuda.current_stream(dev).cuda_stream), None)

    def last_redone(self, n_query):
        """diagnostics (synchronises; needs keep_workspace): queries of the last packed scan that were redone exactly --
        by the one-launch finisher's own redo branch (ws_delta[q] == 1) or, on the routes that end with the flag-gated
        exact kernel (the large-batch routes, the pools, the three-launch path: ws_delta holds a selection band there),
        by that kernel, which leaves kRedoneMark = -1 (csrc/scan_args.h).  None on the reference-layout route, which
        writes no ws_delta."""
        ws = self.last_workspace
        route = self.last_route()
        if ws is None or route in (None, "reference_layout", "rejected"):
            return None
        off = (n_query * 4 + 255) // 256 * 256
        d = ws[off:off + 4 * n_query].view(torch.float32)
        return int((d == (1.0 if route == "one_launch_finish" else -1.0)).sum().item())

    ROUTES = {0: "reference_layout", 1: "one_launch_finish", 2: "sorted_lists", 3: "pools", 8: "dump_f32",
              16: "dump_sel16", 17: "dump_sel16_w8", -1: "rejected"}

    def route(self, n_query, k, n_split=1, ds=0, n_probe=1, slots_hint=None, has_lut=True, packed=True,
              tickets=None, residual=False):
        """diagnostics: the kernels a call with these arguments runs (tpq_ivfpq_scan_route: the library's own rule,
        nothing is launched) -- one of ROUTES' names.  `tickets` defaults to what topk / topk_fused pass: the cached
        buffer of a split query outside a stream capture."""
        if tickets is None:
            tickets = n_split > 1
        code = load().tpq_ivfpq_scan_route(int(n_query), int(k), int(n_split), self.m, int(ds), int(n_probe),
                                            int(slots_hint or 0), int(bool(has_lut)),
                                            int(bool(packed) and self.m in PACKED_M), int(bool(tickets)),
                                            int(bool(residual)))
        return self.ROUTES.get(code, str(code))

    def last_route(self):
        """diagnostics: route(...) of the last topk / topk_fused call"""
        return None if self.last_call is None else self.route(**self.last_call)

    def ordered(self, workspace_bytes, slots=0):
        """diagnostics: whether the last topk / topk_fused call, handed `workspace_bytes` of workspace, dispatches its
        queries longest first (tpq_ivfpq_scan_ordered: the library's own rule, nothing is launched; `slots`: the
        device's workgroup slots, 0 = ask the device the call ran on)"""
        if self.last_call is None:
            return None
        c = self.last_call
        with torch.cuda.device(self._last_device):
            code = load().tpq_ivfpq_scan_ordered(int(c["n_query"]), int(c["k"]), int(c["n_split"]), self.m, int(c["ds"]),
                                                  int(c["n_probe"]), int(c["slots_hint"] or 0), int(bool(c["has_lut"])),
                                                  int(bool(c["packed"]) and self.m in PACKED_M), int(c["n_split"] > 1),
                                                  int(bool(c.get("residual", False))), int(slots), int(workspace_bytes))
        return code == 1

    def last_ordered(self):
        """diagnostics: whether the last topk / topk_fused call dispatched its queries longest first (csrc/scan_order.hip:
        a large batch of more than one round of workgroup slots whose workspace has room for the order)"""
        return None if self.last_call is None else self.ordered(self.last_workspace_bytes)

    def _cell_query(self, name, workspace_bytes, n_cells, n_slots):
        if self.last_call is None:
            return None
        c = self.last_call
        code = getattr(load(), name)(int(c["n_query"]), int(c["k"]), int(c["n_split"]), self.m, int(c["ds"]),
                                     int(c["n_probe"]), int(c["slots_hint"] or 0), int(bool(c["has_lut"])),
                                     int(bool(c["packed"]) and self.m in PACKED_M), int(c["n_split"] > 1),
                                     int(bool(c.get("residual", False))), int(n_cells), int(n_slots),
                                     int(workspace_bytes))
        return code == 1

    def cell_major(self, workspace_bytes, n_cells, n_slots):
        """diagnostics: whether the last topk_fused call, handed `workspace_bytes` of workspace and the probed cells of
        an index of `n_cells` cells over `n_slots` slots, takes the cell-major form of the large-batch route
        (tpq_ivfpq_scan_cell_major: the library's own rule, nothing is launched)"""
        return self._cell_query("tpq_ivfpq_scan_cell_major", workspace_bytes, n_cells, n_slots)

    def cell_norms(self, workspace_bytes, n_cells, n_slots):
        """diagnostics: whether such a call takes the form AND its candidate kernel reads the slot norms of an array
        computed once per call -- the workspace has room for it behind the lists and inversion arrays in use -- and does
        not form them in every block (tpq_ivfpq_scan_cell_norms: the library's own rule, nothing is launched)"""
        return self._cell_query("tpq_ivfpq_scan_cell_norms", workspace_bytes, n_cells, n_slots)

    def last_cell_major(self):
        """diagnostics: whether the last topk / topk_fused call ran the cell-major form (csrc/scan_cells.hip): it handed
        over its cells and the library's rule took them"""
        if self.last_call is None:
            return None
        if self._last_cells is None:
            return False
        return self.cell_major(self.last_workspace_bytes, *self._last_cells)

    def last_cell_norms(self):
        """diagnostics: whether the last topk / topk_fused call ran the cell-major form with per-call slot norms
        (cell_norm_kernel, csrc/scan_cells.hip); False where last_cell_major() is"""
        if self.last_call is None:
            return None
        if self._last_cells is None:
            return False
        return self.cell_norms(self.last_workspace_bytes, *self._last_cells)

    def cell_threshold(self, workspace_bytes, n_cells, n_slots):
        """diagnostics: whether such a call takes the cell-major form's threshold form -- no query-major pass, the
        threshold from group maxima of the candidate kernel's own values (tpq_ivfpq_scan_cell_threshold: the library's
        own rule, nothing is launched)"""
        return self._cell_query("tpq_ivfpq_scan_cell_threshold", workspace_bytes, n_cells, n_slots)

    def last_cell_threshold(self):
        """diagnostics: whether the last topk / topk_fused call ran the cell-major form's threshold form
        (csrc/scan_cells.hip); False where last_cell_norms() is, and for a call that switched it off
        (cell_threshold=False)"""
        if self.last_call is None:
            return None
        if self._last_cells is None or self._last_withheld:
            return False
        return self.cell_threshold(self.last_workspace_bytes, *self._last_cells)

    def last_cell_products(self):
        """diagnostics: the fp16 MFMA products per k-step the candidate kernels of the last topk / topk_fused call ran
        (tpq_ivfpq_scan_last_cell_products, read right after the call): 1 -- the threshold form's single-product key
        and its per-query band (csrc/scan_cells.hip, `The single-product key`; ds = 2 with the switch on) --, 3, or 0
        for a call that did not take the cell-major form"""
        return self._last_products

    def last_cell_threshold_state(self):
        """diagnostics (synchronises; needs keep_workspace and a last call that ran the threshold form): what the form's
        first pass and cell_kth_kernel left in the workspace, as a dict of
          count      i32 [nq]       maxima the first pass reserved room for (beyond the capacity: dropped)
          maxima     f32 [nq, cap]  entry e of a query's list as a fast value: NaN for a group without a live slot, -inf
                                    past min(count, cap)
          survived   bool [nq, cap] the entry is still the first pass's: the list is filled from the END of the query's key
                                    area downwards, the candidates from its front, which overwrote the others
          threshold  f32 [nq]       what the candidate pass tested against: M_k - 2 delta_q, folded over |q|^2 when
                                    euclidean (tpq_ivfpq_cell_fold_threshold); +inf for a flagged query
          band       f32 [nq]       2 delta_q (-1 for a query redone exactly);  qnorm f32 [nq]: |q|^2
          candidates i32 [nq]       entries the candidate pass appended (beyond the capacity: counted, not stored)"""
        assert self.last_workspace is not None and self.last_cell_threshold() is True
        ws, c = self.last_workspace, self.last_call
        nq, k, n_probe = c["n_query"], c["k"], c["n_probe"]
        n_cells, n_slots = self._last_cells
        align = lambda n: (n + 255) // 256 * 256  # noqa: E731
        lists = lambda ch: 2 * align(nq * 4) + nq * ch * 512 + align(nq * ch * 4)  # noqa: E731
        extras = load().tpq_ivfpq_cell_candidates_workspace_bytes(nq, n_probe, n_cells, 4)   # (kCellP0's layout)
        chunks = next(ch for ch in (16, 8) if (k + 63) // 64 < ch and self.last_workspace_bytes >= lists(ch) + extras)
        cap = chunks * 64

        def arr(off, n, dtype):
            return ws[off:off + 4 * n].view(dtype)
        band = arr(align(nq * 4), nq, torch.float32).clone()
        keys = arr(2 * align(nq * 4), nq * cap, torch.int32).view(nq, cap)
        ex = lists(chunks) + 256
        thr, qnorm, cand = (arr(ex + i * align(nq * 4), nq, t).clone()
                            for i, t in ((0, torch.float32), (2, torch.float32), (3, torch.int32)))
        # behind the extras and the norms: pass B's pairs, pass A's inversion, then the counts (csrc/scan_cells.h)
        t_probes = load().tpq_ivfpq_scan_cell_threshold_probes()
        off = (lists(chunks) + extras + align(n_slots * 4) + align(nq * n_probe * 4) + 3 * align(n_cells * 4)
               + 2 * align((n_cells + 1) * 4) + align(nq * min(t_probes, n_probe) * 4))
        count = arr(off, nq, torch.int32).clone()
        e = torch.arange(cap, device=ws.device)[None, :]
        stored = e < count.clamp(max=cap)[:, None]
        rev = keys.flip(1)                                   # entry e is position cap - 1 - e
        bits = torch.where(rev < 0, rev & 0x7fffffff, ~rev).view(torch.float32)
        maxima = torch.where(stored, bits, torch.full_like(bits, -float("inf")))
        maxima = torch.where(stored & (rev == 0), torch.full_like(bits, float("nan")), maxima)
        survived = stored & (cap - 1 - e >= cand.clamp(max=cap)[:, None])
        return dict(count=count, maxima=maxima, survived=survived, threshold=thr, band=band, qnorm=qnorm,
                    candidates=cand)

    def _n_split(self, n_query, device, slots_hint=None):
        """Workgroups per query so that small batches still fill the chip (256 CUs x 2), see workgroups_per_query."""
        if self.n_cus is None:
            self.n_cus = torch.cuda.get_device_properties(device).multi_processor_count
        # four 4-wave workgroups per CU for short codes (m <= 32), two 8-wave ones while the LUT is
        # <= 64 KiB, one 16-wave workgroup above (csrc/scan_packed_kernel.h packed_waves)
        per_cu, waves = (4, 4) if self.m <= 32 else (2, 8) if self.m <= 64 else (1, 16)
        return workgroups_per_query(n_query, self.n_cus, per_cu, waves, slots_hint)

    def _scan(self, name, inputs, data, cell_start, address2id, k, n_split, slots_hint, packed, ticketed,
              cells=None, n_cells=0, cell_threshold=True, kept=None, cell_single_product=True, **route):
        """What topk / topk_fused / topk_residual_packed share once their arguments are checked: the outputs, the
        split, the diagnostics, the workspace and the call of `name` -- its own `inputs`, then the arguments every
        scan entry point of the library ends with (`ticketed`: the symbol takes tickets and the slots hint; `cells`:
        it takes the probed cells and their number behind those; `kept`: see topk_fused)."""
        n_data, device = data.shape[1], data.device
        n_query, n_probe = cell_start.shape
        values, address, ids = alloc_topk(n_query, k, device, address2id)
        if n_query == 0:
            return topk_result(values, address, ids)
        lib = load()
        if n_split is None:
            n_split = self._n_split(n_query, device, slots_hint)
        self.last_n_split = n_split  # diagnostics / tests: workgroups per query of the last call
        self.last_call = dict(n_query=n_query, k=k, n_split=n_split, n_probe=n_probe, slots_hint=slots_hint,
                              packed=packed is not None, **route)
        self._last_cells = (int(n_cells), int(n_data)) if cells is not None else None
        self._last_withheld = not cell_threshold
        ws_bytes = lib.tpq_ivfpq_scan_workspace_bytes(n_query, k, n_split, self.m)
        if self.workspace_bytes is not None:
            ws_bytes = int(self.workspace_bytes)
        self.last_workspace_bytes, self._last_device = ws_bytes, device
        ws = torch.empty(max(ws_bytes, 1), device=device, dtype=torch.uint8)
        # the kept state: asked for only when the library's own rule takes the form with slot norms for this call (a
        # state is 4 bytes per slot), and never built inside a capture: such a call takes the per-call path
        self.last_cell_kept = None
        if kept is not None and cells is not None and self.cell_norms(ws_bytes, n_cells, n_data):
            kept = kept(lib.tpq_ivfpq_cell_kept_bytes(int(n_data), int(route["ds"])), device)
            if kept is not None and not kept.valid and torch.cuda.is_current_stream_capturing():
                kept = None
        else:
            kept = None
        ev = None
        if self.record_events is not None:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record(torch.cuda.current_stream(device))
        with torch.cuda.device(device):
            tail = ()
            if ticketed:
                tickets = self._tickets(n_query, n_split, device) if packed is not None else None
                tail = (ptr(tickets), int(slots_hint or 0))
                if cells is not None:
                    tail += (ptr(cells), int(n_cells))
                if kept is not None:
                    name = "tpq_ivfpq_search_fused_cells_kept"
                    kept.before_use(device)
                    tail += (ptr(kept.buf), kept.buf.numel(), int(kept.valid))
            # (the switch is the library's, process-wide and read on the host during the call: set for this call alone)
            before = lib.tpq_ivfpq_scan_use_cell_threshold(1 if cell_threshold else 0)
            before_sp = lib.tpq_ivfpq_scan_use_cell_single_product(1 if cell_single_product else 0)
            try:
                rc = getattr(lib, name)(*inputs, ptr(values), ptr(address), ptr(address2id), ptr(ids), n_data, n_query,
                                        n_probe, self.m, k, n_split, ptr(ws), ws_bytes, *tail, stream_ptr(device))
                self._last_products = lib.tpq_ivfpq_scan_last_cell_products()
            finally:
                lib.tpq_ivfpq_scan_use_cell_threshold(before)
                lib.tpq_ivfpq_scan_use_cell_single_product(before_sp)
            if rc != 0 and ticketed:
                self._drop_tickets(device)
            check(rc, name)
            if kept is not None:
                self.last_cell_kept = "reused" if kept.valid else "built"
                if not kept.valid:
                    kept.after_build(device)
        if self.keep_workspace:
            self.last_workspace = ws
        if ev is not None:
            ev[1].record(torch.cuda.current_stream(device))
            self.record_events.append(ev)
        return topk_result(values, address, ids)

    def topk(self, data, precomputed, is_empty, cell_start, cell_size, n_probe_list,
             n_candidates=None, packed=None, address2id=None, n_split=None, slots_hint=None):
        """
          data: [m // 4, n_data, 4] uint8           (CellContainer._storage)
          precomputed: [m, n_query, 256] float32    (PQCodec.precompute_adc)
          is_empty: [n_data] uint8, or None when no slot inside a cell is a tombstone
          cell_start / cell_size: [n_query, max_n_probe] int64
          n_probe_list: [n_query] int64
          n_candidates: k of the top-k (<= 1024)
          packed: optional scan-layout copy of `data` (enables the bank-conflict-free kernel)
          address2id: optional [n_data] int64; when given a third tensor (ids) is returned
        returns (values [n_query, k] descending, address [n_query, k][, ids])
        """
        n_data = data.shape[1]
        n_query, n_probe = cell_start.shape
        assert precomputed.shape == (self.m, n_query, self.k)
        assert data.shape[0] == self.m // self.n_cs
        assert data.shape[2] == self.n_cs
        assert cell_size.shape[1] == n_probe
        assert data.dtype == torch.uint8
        assert precomputed.dtype == torch.float32
        assert cell_start.dtype == cell_size.dtype == torch.int64
        assert n_probe_list.shape == (n_query,)
        assert n_probe_list.dtype == torch.int64
        if is_empty is not None:
            assert is_empty.shape[0] == n_data
            assert is_empty.dtype == torch.uint8
        if n_candidates is None:
            n_candidates = self.tpb
        assert 0 < n_candidates <= 1024
        require_gpu(data, precomputed, is_empty, cell_start, cell_size, n_probe_list, packed,
                    address2id)
        inputs = (ptr(data), ptr(precomputed), ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list))
        if packed is not None and self.m in PACKED_M:
            return self._scan("tpq_ivfpq_scan_topk_packed_tickets", (ptr(packed), *inputs), data, cell_start,
                              address2id, n_candidates, n_split, slots_hint, packed, True, ds=0, has_lut=True)
        return self._scan("tpq_ivfpq_scan_topk", inputs, data, cell_start, address2id, n_candidates, n_split,
                          slots_hint, packed, False, ds=0, has_lut=True)

    def topk_fused(self, data, query, codebook, is_empty, cell_start, cell_size, n_probe_list,
                   n_candidates, distance="euclidean", packed=None, address2id=None, n_split=None,
                   slots_hint=None, cells=None, n_cells=0, cell_threshold=True, kept=None, cell_single_product=True):
        """precompute_adc + topk in one pass: the LUT is built inside the scan workgroups
        (query [d, n_query] f32, codebook [m, ds, 256] f32); results identical to
        topk(precomputed=AdcLutHip()(query, codebook)).  `cells` [n_query, max_n_probe] int64 -- the probed cells
        behind cell_start / cell_size, ids in [0, n_cells) -- lets a cell-dense large batch at m = 64 take the
        cell-major form (tpq_ivfpq_search_fused_cells; `last_cell_major()`): same results.  `cell_threshold=False`
        keeps that form to its seeded variant (tpq_ivfpq_scan_use_cell_threshold; `last_cell_threshold()`).
        `cell_single_product=False` keeps the threshold form's selection key on three fp16 products per k-step
        (tpq_ivfpq_scan_use_cell_single_product; `last_cell_products()`): same results, a narrower band -- for data with
        many rows within the single product's band of the k-th best, whose lists would overflow.
        `kept`: a callable (n_bytes, device) -> CellKeptState or None, asked only when the call takes that form with slot
        norms: the state of what the form derives from `data`, `codebook` and `is_empty` alone, built by the first call
        that finds it not valid and read by the others (tpq_ivfpq_search_fused_cells_kept; `last_cell_kept`: "built",
        "reused" or None).  The caller answers for the state matching those three tensors."""
        n_data = data.shape[1]
        n_query, n_probe = cell_start.shape
        m, ds, kk = codebook.shape
        assert m == self.m and kk == self.k
        assert query.shape == (m * ds, n_query)
        assert query.dtype == codebook.dtype == torch.float32
        assert data.shape == (self.m // self.n_cs, n_data, self.n_cs) and data.dtype == torch.uint8
        assert cell_size.shape == (n_query, n_probe)
        assert cell_start.dtype == cell_size.dtype == torch.int64
        assert n_probe_list.shape == (n_query,) and n_probe_list.dtype == torch.int64
        assert 0 < n_candidates <= 1024
        query = query.contiguous()
        codebook = codebook.contiguous()
        require_gpu(data, query, codebook, is_empty, cell_start, cell_size, n_probe_list, packed,
                    address2id)
        inputs = (ptr(packed), ptr(data), ptr(query), ptr(codebook), ds, metric_code(distance), ptr(is_empty),
                  ptr(cell_start), ptr(cell_size), ptr(n_probe_list))
        if cells is not None:
            assert cells.shape == (n_query, n_probe) and cells.dtype == torch.int64 and n_cells >= 1
            cells = cells.contiguous()
            require_gpu(cells)
            return self._scan("tpq_ivfpq_search_fused_cells", inputs, data, cell_start, address2id, n_candidates,
                              n_split, slots_hint, packed, True, cells=cells, n_cells=n_cells, cell_threshold=cell_threshold,
                              kept=kept, cell_single_product=cell_single_product, ds=ds, has_lut=False)
        return self._scan("tpq_ivfpq_search_fused_tickets", inputs, data, cell_start, address2id, n_candidates,
                          n_split, slots_hint, packed, True, ds=ds, has_lut=False)

    # ---- residual PQ (pq_use_residual=True) ------------------------------------------------------
    def _residual(self, data, part1, part2, full, cells, base_sims, is_empty, cell_start, cell_size,
                  n_probe_list, n_candidates, address2id):
        n_data = data.shape[1]
        n_query, n_probe = cell_start.shape
        assert data.shape == (self.m // self.n_cs, n_data, self.n_cs)
        assert cell_size.shape == (n_query, n_probe)
        assert base_sims.shape == (n_query, n_probe)
        assert data.dtype == torch.uint8
        assert cell_start.dtype == cell_size.dtype == torch.int64
        assert base_sims.dtype == torch.float32
        assert n_probe_list.shape == (n_query,)
        assert n_probe_list.dtype == torch.int64
        if is_empty is not None:
            assert is_empty.shape == (n_data,) and is_empty.dtype == torch.uint8
        if n_candidates is None:
            n_candidates = self.tpb
        assert 0 < n_candidates <= 1024
        # logical [q][j][c] / [cell][j][c] / [q][p][j][c] order, whatever view the caller built
        part1 = None if part1 is None else part1.contiguous()
        part2 = None if part2 is None else part2.contiguous()
        full = None if full is None else full.contiguous()
        cells = None if cells is None else cells.contiguous()
        base_sims = base_sims.contiguous()
        require_gpu(data, part1, part2, full, cells, base_sims, is_empty, cell_start, cell_size,
                    n_probe_list, address2id)
        k = n_candidates
        values, address, ids = alloc_topk(n_query, k, data.device, address2id)
        if n_query:
            call("tpq_ivfpq_scan_topk_residual", data.device,
                 ptr(data), ptr(part1), ptr(part2), ptr(full), ptr(cells), ptr(base_sims),
                 ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list), ptr(values),
                 ptr(address), ptr(address2id), ptr(ids), n_data, n_query, n_probe, self.m, k)
        return topk_result(values, address, ids)

    def topk_residual_packed(self, data, packed, part2, slot_term, cell_bound, cells, base_sims,
                             is_empty, cell_start, cell_size, n_probe_list, n_candidates,
                             part1=None, query=None, codebook=None, address2id=None, n_split=None,
                             slots_hint=None):
        """Residual scan on the scan layout (tpq_ivfpq_scan_topk_residual_packed): results equal
        topk_residual_precomputed bit for bit.  part1 [n_query, m, 256] or (query [d, n_query],
        codebook [m, ds, 256]) from which the workgroup builds it; part2 [n_cells, m, 256]
        contiguous; slot_term / cell_bound from ResidualSlotTermsHip."""
        n_data = data.shape[1]
        n_query, n_probe = cell_start.shape
        assert self.m in PACKED_M and packed is not None
        assert data.shape == (self.m // self.n_cs, n_data, self.n_cs) and data.dtype == torch.uint8
        assert part2.shape[1:] == (self.m, self.k) and part2.dtype == torch.float32
        assert part2.is_contiguous()
        assert slot_term.shape == (n_data,) and slot_term.dtype == torch.float32
        assert cell_bound.shape == (part2.shape[0],) and cell_bound.dtype == torch.float32
        assert cells.shape == cell_start.shape == cell_size.shape == base_sims.shape
        assert cells.dtype == cell_start.dtype == cell_size.dtype == torch.int64
        assert base_sims.dtype == torch.float32
        assert n_probe_list.shape == (n_query,) and n_probe_list.dtype == torch.int64
        assert 0 < n_candidates <= 1024
        ds = 0
        if part1 is not None:
            assert part1.shape == (n_query, self.m, self.k) and part1.dtype == torch.float32
            part1 = part1.contiguous()
        else:
            assert query is not None and codebook is not None
            ds = codebook.shape[1]
            assert codebook.shape == (self.m, ds, self.k) and query.shape == (self.m * ds, n_query)
            assert query.dtype == codebook.dtype == torch.float32
            query = query.contiguous()
            codebook = codebook.contiguous()
        cells = cells.contiguous()
        base_sims = base_sims.contiguous()
        require_gpu(data, packed, part1, query, codebook, part2, slot_term, cell_bound, cells,
                    base_sims, is_empty, cell_start, cell_size, n_probe_list, address2id)
        inputs = (ptr(packed), ptr(data), ptr(part1), ptr(query), ptr(codebook), ds, ptr(part2), ptr(slot_term),
                  ptr(cell_bound), ptr(cells), ptr(base_sims), ptr(is_empty), ptr(cell_start), ptr(cell_size),
                  ptr(n_probe_list))
        return self._scan("tpq_ivfpq_scan_topk_residual_packed", inputs, data, cell_start, address2id,
                          n_candidates, n_split, slots_hint, packed, False, ds=ds, has_lut=part1 is not None,
                          residual=True)

    def topk_residual(self, data, precomputed, base_sims, is_empty, cell_start, cell_size,
                      n_probe_list, n_candidates=None, address2id=None):
        """precomputed: [n_query, max_n_probe, m, 256] f32 -- one LUT per (query, probe)
        (kernels/IVFPQTopkCuda.py:144-210)."""
        n_query, n_probe = cell_start.shape
        assert precomputed.shape == (n_query, n_probe, self.m, self.k)
        assert precomputed.dtype == torch.float32
        return self._residual(data, None, None, precomputed, None, base_sims, is_empty, cell_start,
                              cell_size, n_probe_list, n_candidates, address2id)

    def topk_residual_precomputed(self, data, part1, part2, cells, base_sims, is_empty, cell_start,
                                  cell_size, n_probe_list, n_candidates=None, address2id=None):
        """part1 [n_query, m, 256], part2 [n_cells, m, 256] f32, cells [n_query, max_n_probe] int64
        (kernels/IVFPQTopkCuda.py:212-283)."""
        n_query = cell_start.shape[0]
        assert part1.shape == (n_query, self.m, self.k) and part2.shape[1:] == (self.m, self.k)
        assert part1.dtype == part2.dtype == torch.float32
        assert cells.shape == cell_start.shape and cells.dtype == torch.int64
        return self._residual(data, part1, part2, None, cells, base_sims, is_empty, cell_start,
                              cell_size, n_probe_list, n_candidates, address2id)


class CellCandidatesHip:
    """The cell-major candidate pass on its own (tpq_ivfpq_cell_candidates, csrc/scan_cells.hip): for the probes
    first_probe <= p < n_probe_list[q] of every query, every live slot whose fp16 matrix-core value is >= threshold[q] -
    delta_q; m = 64, sub-vectors of 1 or 2 components."""

    def __call__(self, data, query, codebook, cells, n_cells, cell_start, cell_size, n_probe_list, threshold,
                 first_probe=0, capacity=1024, is_empty=None, distance="euclidean", slot_norms=True):
        """-> (count i32 [nq], values f32 [nq, capacity], address i64 [nq, capacity] (-1 past the count), band f32 [nq]
        = 2 delta_q, flags i32 [nq]).  slot_norms: hand over the workspace with room for the per-call slot norms
        (tpq_ivfpq_cell_candidates_norms_workspace_bytes); False: exactly tpq_ivfpq_cell_candidates_workspace_bytes, and
        the candidate kernel forms the norms itself.  The same candidates with the same values either way."""
        m, ds, kk = codebook.shape
        n_data = data.shape[1]
        n_query, n_probe = cell_start.shape
        assert m == 64 and kk == 256 and ds in (1, 2) and query.shape == (m * ds, n_query)
        assert data.shape == (16, n_data, 4) and data.dtype == torch.uint8
        assert cells.shape == cell_size.shape == (n_query, n_probe)
        assert cells.dtype == cell_start.dtype == cell_size.dtype == n_probe_list.dtype == torch.int64
        assert threshold.shape == (n_query,) and threshold.dtype == torch.float32
        query, codebook, cells = query.contiguous(), codebook.contiguous(), cells.contiguous()
        require_gpu(data, query, codebook, cells, is_empty, cell_start, cell_size, n_probe_list, threshold)
        dev = data.device
        count = torch.zeros(n_query, device=dev, dtype=torch.int32)
        keys = torch.zeros(n_query, capacity, device=dev, dtype=torch.int32)
        addr = torch.zeros(n_query, capacity, device=dev, dtype=torch.int32)
        band = torch.zeros(n_query, device=dev, dtype=torch.float32)
        flags = torch.zeros(n_query, device=dev, dtype=torch.int32)
        if slot_norms:
            ws_bytes = load().tpq_ivfpq_cell_candidates_norms_workspace_bytes(n_query, n_probe, int(n_cells),
                                                                              int(first_probe), n_data)
        else:
            ws_bytes = load().tpq_ivfpq_cell_candidates_workspace_bytes(n_query, n_probe, int(n_cells), int(first_probe))
        ws = torch.empty(max(ws_bytes, 1), device=dev, dtype=torch.uint8)
        call("tpq_ivfpq_cell_candidates", dev, ptr(data), ptr(query), ptr(codebook), ds, metric_code(distance),
             ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list), ptr(cells), int(n_cells),
             int(first_probe), ptr(threshold), n_data, n_query, n_probe, m, int(capacity), ptr(count), ptr(keys),
             ptr(addr), ptr(band), ptr(flags), ptr(ws), ws_bytes)
        address = (~addr).to(torch.int64)
        stored = torch.arange(capacity, device=dev)[None, :] < count.clamp(max=capacity)[:, None]
        address = torch.where(stored, address, torch.full_like(address, -1))
        neg = keys < 0                                  # (the image's top bit: a value >= 0)
        bits = torch.where(neg, keys & 0x7fffffff, ~keys)
        values = torch.where(stored, bits.view(torch.float32), torch.full_like(band[:, None].expand_as(bits), -float("inf")))
        return count, values, address, band, flags


class ScanOrderHip:
    """The dispatch order of a large batch on its own (tpq_ivfpq_scan_order, csrc/scan_order.hip): the queries by the
    tiles of 2^tile_shift slots they scan, longest first -- what the large-batch scan routes compute per call."""

    def __call__(self, cell_start, cell_size, n_probe_list, tile_shift=6):
        """cell_start / cell_size [n_query, max_n_probe] int64, n_probe_list [n_query] int64 -> (order, rank, work),
        int32 [n_query] each: work non-increasing along order, equal work by ascending query; rank[order[i]] == i"""
        n_query, n_probe = cell_start.shape
        assert cell_size.shape == (n_query, n_probe) and n_probe >= 1
        assert cell_start.dtype == cell_size.dtype == torch.int64
        assert n_probe_list.shape == (n_query,) and n_probe_list.dtype == torch.int64
        require_gpu(cell_start, cell_size, n_probe_list)
        order, rank, work = (torch.empty(n_query, device=cell_start.device, dtype=torch.int32) for _ in range(3))
        if n_query:
            call("tpq_ivfpq_scan_order", cell_start.device, ptr(cell_start), ptr(cell_size), ptr(n_probe_list),
                 n_query, n_probe, int(tile_shift), ptr(order), ptr(rank), ptr(work))
        return order, rank, work


class ResidualSlotTermsHip:
    """Per-slot / per-cell constants of the packed residual scan (tpq_ivfpq_residual_slot_terms):
    slot_term [n_data] f32 = sum_j part2[cell(s), j, code_j(s)], cell_bound [n_cells] f32."""

    def __call__(self, data, part2, cell_start, cell_size):
        n_cells, m, kk = part2.shape
        n_data = data.shape[1]
        assert kk == 256 and data.shape == (m // 4, n_data, 4) and data.dtype == torch.uint8
        assert part2.dtype == torch.float32 and part2.is_contiguous()
        assert cell_start.shape == cell_size.shape == (n_cells,)
        assert cell_start.dtype == cell_size.dtype == torch.int64
        require_gpu(data, part2, cell_start, cell_size)
        slot_term = torch.empty(n_data, device=data.device, dtype=torch.float32)
        cell_bound = torch.empty(n_cells, device=data.device, dtype=torch.float32)
        call("tpq_ivfpq_residual_slot_terms", data.device, ptr(data), ptr(part2), ptr(cell_start), ptr(cell_size),
             ptr(slot_term), ptr(cell_bound), n_data, n_cells, m)
        return slot_term, cell_bound


class ResidualPart1Hip:
    """part1[q, j, c] = 2 * q_j . r_jc (index/IVFPQIndex.py:366-379), [n_query, m, 256] f32."""

    def __call__(self, query, codebook):
        m, ds, k = codebook.shape
        assert k == 256 and query.shape[0] == m * ds
        query = query.contiguous()
        codebook = codebook.contiguous()
        require_gpu(query, codebook)
        nq = query.shape[1]
        out = torch.empty(nq, m, 256, device=query.device, dtype=torch.float32)
        call("tpq_residual_part1", query.device, ptr(query), ptr(codebook), ptr(out), m, ds, nq)
        return out


class IVFPQTop1Hip(IVFPQTopkHip):
    """k = 1 variant (kernels/IVFPQTop1Cuda.py:86-140): same kernel family, list of one."""

    def topk(self, *args, n_candidates=1, **kwargs):
        return super().topk(*args, n_candidates=n_candidates, **kwargs)


class AdcLutHip:
    """PQCodec.precompute_adc on the fp32 matrix cores (codec/PQCodec.py:62-75)."""

    def __call__(self, query, codebook, distance="euclidean"):
        """query [d, n_query] f32, codebook [m, ds, 256] f32 -> [m, n_query, 256] f32"""
        m, ds, k = codebook.shape
        assert k == 256
        assert query.shape[0] == m * ds
        assert query.dtype == codebook.dtype == torch.float32
        query = query.contiguous()
        codebook = codebook.contiguous()
        require_gpu(query, codebook)
        nq = query.shape[1]
        lut = torch.empty(m, nq, 256, device=query.device, dtype=torch.float32)
        if nq == 0:   # (an empty tensor has no address to hand to the library)
            return lut
        call("tpq_adc_lut", query.device, ptr(query), ptr(codebook), ptr(lut), m, ds, nq, metric_code(distance))
        return lut


class IVFPQRerankHip:
    """The re-rank step of IVFPQRIndex (tpq_ivfpqr_rerank; the second half of the legacy IVFPQR.topk,
    legacy/IVFPQR.py:408-473): the candidates of the list scan re-valued from both codes of their slot,
    the best k kept."""

    def __call__(self, storage, n_subvectors, codebook, codebook_r, query, cand_address, k, use_residual=True,
                 distance="euclidean", address2id=None):
        """
          storage: [(m + m_r) // 4, capacity, 4] uint8, first the m first-stage rows, then the m_r re-rank rows
          codebook [m, ds, 256] / codebook_r [m_r, ds_r, 256] float32 (codebook may be None when not use_residual)
          query: [d, n_query] float32 (normalised by the caller for "cosine")
          cand_address: [n_query, k1] int64, -1 = no candidate
          address2id: optional [capacity] int64; when given a third tensor (ids) is returned
        returns (values [n_query, k] descending, address [n_query, k][, ids]); unfilled = (-inf, -1, -1)
        """
        m = n_subvectors
        g, capacity, cs = storage.shape
        m_r, ds_r, kk = codebook_r.shape
        d, n_query = query.shape
        k1 = cand_address.shape[1]
        assert cs == 4 and storage.dtype == torch.uint8 and g * 4 == m + m_r
        assert kk == 256 and d == m_r * ds_r and d % m == 0
        assert cand_address.shape == (n_query, k1) and cand_address.dtype == torch.int64
        assert query.dtype == codebook_r.dtype == torch.float32
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= k1 <= 1024
        if use_residual:
            assert codebook.shape == (m, d // m, 256) and codebook.dtype == torch.float32
            codebook = codebook.contiguous()
        else:
            codebook = None
        if address2id is not None:
            assert address2id.shape == (capacity,) and address2id.dtype == torch.int64
        query = query.contiguous()
        codebook_r = codebook_r.contiguous()
        cand_address = cand_address.contiguous()
        require_gpu(storage, codebook, codebook_r, query, cand_address, address2id)
        values, address, ids = alloc_topk(n_query, k, storage.device, address2id)
        if n_query:
            call("tpq_ivfpqr_rerank", storage.device,
                 ptr(storage), capacity, m, m_r, ptr(codebook), ptr(codebook_r), ptr(query), d, n_query,
                 ptr(cand_address), k1, k, int(bool(use_residual)), metric_code(distance), ptr(address2id),
                 ptr(values), ptr(address), ptr(ids))
        return topk_result(values, address, ids)


# ---- what the list-scan wrappers share -----------------------------------------------------------------------------
def _check_lists(n_data, is_empty, cell_start, cell_size, n_probe_list):
    """the list arguments of a scan over a storage of n_data slots -> (n_query, n_probe)"""
    n_query, n_probe = cell_start.shape
    assert cell_size.shape == (n_query, n_probe) and n_probe >= 1
    assert cell_start.dtype == cell_size.dtype == torch.int64
    assert n_probe_list.shape == (n_query,) and n_probe_list.dtype == torch.int64
    if is_empty is not None:
        assert is_empty.shape == (n_data,) and is_empty.dtype == torch.uint8
    return n_query, n_probe


def _split_and_workspace(scan, workspace_bytes, n_query, k, n_split, slots_hint, device):
    """What the IVFFlat and IVFPQ4 top-k wrappers do before their call, for a batch that is not empty: pick n_split
    (recorded in scan.last_n_split) and size the workspace with the library's `workspace_bytes(n_query, k, n_split)`.
    Returns (n_split, ws, ws_bytes)."""
    if n_split is None:
        n_split = scan._n_split(n_query, device, slots_hint)
    scan.last_n_split = n_split
    ws_bytes = workspace_bytes(n_query, k, n_split)
    ws = torch.empty(ws_bytes, device=device, dtype=torch.uint8) if ws_bytes else None
    return n_split, ws, ws_bytes


class IVFFlatTopkHip:
    """The list scan of IVFFlatIndex (tpq_ivfflat_scan_topk, csrc/scan_flat.hip): the probed cells hold the vectors
    themselves; value and order are defined in include/torchpq_amd.h."""

    def __init__(self):
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last call

    def _n_split(self, n_query, device, slots_hint=None):
        """Workgroups per query: two 8-wave workgroups per CU, see workgroups_per_query."""
        if self.n_cus is None:
            self.n_cus = torch.cuda.get_device_properties(device).multi_processor_count
        return workgroups_per_query(n_query, self.n_cus, 2, 8, slots_hint)

    def __call__(self, vectors, query, cell_start, cell_size, n_probe_list, k, is_empty=None,
                 distance="euclidean", n_split=None, slots_hint=None):
        """
          vectors: [d, n_slots] float32 (or [d, n_slots, 1]: CellContainer._storage.view(torch.float32))
          query: [d, n_query] float32 (normalised by the caller for "cosine")
          cell_start / cell_size: [n_query, max_n_probe] int64; n_probe_list: [n_query] int64
          is_empty: [n_slots] uint8, or None when no slot inside a cell is a tombstone
        returns (values [n_query, k] descending, address [n_query, k]); unfilled = (-inf, -1)
        """
        if vectors.dim() == 3:
            assert vectors.shape[2] == 1
            vectors = vectors[:, :, 0]
        d, n_slots = vectors.shape
        n_query, n_probe = cell_start.shape
        assert query.shape == (d, n_query)
        assert vectors.dtype == query.dtype == torch.float32
        _check_lists(n_slots, is_empty, cell_start, cell_size, n_probe_list)
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= 1024
        query = query.contiguous()
        require_gpu(vectors, query, is_empty, cell_start, cell_size, n_probe_list)
        device = vectors.device
        values, address = alloc_pair(n_query, k, device)
        if n_query == 0:
            return values, address
        n_split, ws, ws_bytes = _split_and_workspace(self, load().tpq_ivfflat_scan_workspace_bytes, n_query, k,
                                                     n_split, slots_hint, device)
        call("tpq_ivfflat_scan_topk", device,
             ptr(vectors), ptr(query), ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list),
             ptr(values), ptr(address), n_slots, d, n_query, n_probe, k, metric_code(distance), n_split, ptr(ws),
             ws_bytes)
        return values, address


class IVFPQ4TopkHip:
    """The list scan of IVFPQ4Index (tpq_ivfpq4_scan_topk, csrc/scan_pq4.hip): 4-bit product-quantized lists, the
    table built inside the scan workgroup; codes, table entry, value and order are defined in include/torchpq_amd.h."""

    def __init__(self, m=8):
        assert m % 8 == 0 and 8 <= m <= 256, "4-bit codes are stored 8 sub-quantizers per word; 8 <= m <= 256"
        self.m = m
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last call

    _n_split = IVFFlatTopkHip._n_split

    def __call__(self, codes, query, codebook, cell_start, cell_size, n_probe_list, k, is_empty=None,
                 distance="euclidean", n_split=None, slots_hint=None):
        """
          codes: [m // 8, n_slots, 4] uint8 (CellContainer._storage of code_size = m // 2)
          query: [d, n_query] float32 (normalised by the caller for "cosine"); codebook: [m, d // m, 16] float32
          cell_start / cell_size: [n_query, max_n_probe] int64; n_probe_list: [n_query] int64
          is_empty: [n_slots] uint8, or None when no slot inside a cell is a tombstone
        returns (values [n_query, k] descending, address [n_query, k]); unfilled = (-inf, -1)
        """
        n_slots = codes.shape[1]
        m, ds, kk = codebook.shape
        n_query, n_probe = cell_start.shape
        assert m == self.m and kk == 16 and ds >= 1
        assert codes.shape == (m // 8, n_slots, 4) and codes.dtype == torch.uint8 and codes.is_contiguous()
        assert query.shape == (m * ds, n_query)
        assert query.dtype == codebook.dtype == torch.float32
        _check_lists(n_slots, is_empty, cell_start, cell_size, n_probe_list)
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= 1024
        query = query.contiguous()
        codebook = codebook.contiguous()
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        require_gpu(codes, query, codebook, is_empty, cell_start, cell_size, n_probe_list)
        device = codes.device
        values, address = alloc_pair(n_query, k, device)
        if n_query == 0:
            return values, address
        n_split, ws, ws_bytes = _split_and_workspace(self, load().tpq_ivfpq4_scan_workspace_bytes, n_query, k,
                                                     n_split, slots_hint, device)
        call("tpq_ivfpq4_scan_topk", device,
             ptr(codes), ptr(query), ptr(codebook), ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list),
             ptr(values), ptr(address), n_slots, m, ds, n_query, n_probe, k, metric_code(distance), n_split, ptr(ws),
             ws_bytes)
        return values, address


class IVFPQ4ResidualTopkHip:
    """The list scan of IVFPQ4Index(pq_use_residual=True) (tpq_ivfpq4_scan_residual_topk, csrc/scan_pq4.hip): 4-bit
    codes of x - centroid(cell); the table of every scanned probe is built inside the scan workgroup from the query,
    the codebook and the probed cell's centroid; defined in include/torchpq_amd.h."""

    def __init__(self, m=8):
        assert m % 8 == 0 and 8 <= m <= 256, "4-bit codes are stored 8 sub-quantizers per word; 8 <= m <= 256"
        self.m = m
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last call

    _n_split = IVFFlatTopkHip._n_split

    def __call__(self, codes, query, codebook, centroids, cells, cell_start, cell_size, n_probe_list, k,
                 is_empty=None, distance="euclidean", n_split=None, slots_hint=None):
        """
          codes, query, codebook, cell_start, cell_size, n_probe_list, is_empty: as IVFPQ4TopkHip
          centroids: [n_cells, d] float32, one coarse centroid per row
          cells: [n_query, max_n_probe] int64, the probed cells (values in [0, n_cells))
        returns (values [n_query, k] descending, address [n_query, k]); unfilled = (-inf, -1)
        """
        n_slots = codes.shape[1]
        m, ds, kk = codebook.shape
        n_query, n_probe = cell_start.shape
        assert m == self.m and kk == 16 and ds >= 1
        assert codes.shape == (m // 8, n_slots, 4) and codes.dtype == torch.uint8 and codes.is_contiguous()
        assert query.shape == (m * ds, n_query)
        assert query.dtype == codebook.dtype == centroids.dtype == torch.float32
        assert centroids.dim() == 2 and centroids.shape[0] >= 1 and centroids.shape[1] == m * ds
        assert cells.shape == (n_query, n_probe) and cells.dtype == torch.int64
        _check_lists(n_slots, is_empty, cell_start, cell_size, n_probe_list)
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= 1024
        query = query.contiguous()
        codebook = codebook.contiguous()
        centroids = centroids.contiguous()
        cells, cell_start, cell_size = cells.contiguous(), cell_start.contiguous(), cell_size.contiguous()
        require_gpu(codes, query, codebook, centroids, cells, is_empty, cell_start, cell_size, n_probe_list)
        device = codes.device
        values, address = alloc_pair(n_query, k, device)
        if n_query == 0:
            return values, address
        n_split, ws, ws_bytes = _split_and_workspace(self, load().tpq_ivfpq4_scan_workspace_bytes, n_query, k,
                                                     n_split, slots_hint, device)
        call("tpq_ivfpq4_scan_residual_topk", device,
             ptr(codes), ptr(query), ptr(codebook), ptr(centroids), ptr(cells), centroids.shape[0], ptr(is_empty),
             ptr(cell_start), ptr(cell_size), ptr(n_probe_list), ptr(values), ptr(address), n_slots, m, ds, n_query,
             n_probe, k, metric_code(distance), n_split, ptr(ws), ws_bytes)
        return values, address


class IVFFlatRangeHip:
    """Range search over the lists of IVFFlatIndex (tpq_ivfflat_range_count / tpq_ivfflat_range_fill,
    csrc/scan_flat.hip): every candidate of IVFFlatTopkHip whose value is >= the query's threshold, in scan order;
    the semantics are defined in include/torchpq_amd.h."""

    def __init__(self):
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last call

    _n_split = IVFFlatTopkHip._n_split

    def __call__(self, vectors, query, cell_start, cell_size, n_probe_list, threshold, is_empty=None,
                 distance="euclidean", n_split=None, slots_hint=None):
        """
          vectors, query, cell_start, cell_size, n_probe_list, is_empty: as IVFFlatTopkHip
          threshold: a Python float, or [n_query] float32 -- one per query
        returns (lims [n_query + 1] int64, values [total] float32, address [total] int64): the hits of query q are
        values[lims[q]:lims[q+1]] / address[lims[q]:lims[q+1]], probe rank ascending, then address ascending.
        Synchronises once: the number of hits sizes the outputs.
        """
        if vectors.dim() == 3:
            assert vectors.shape[2] == 1
            vectors = vectors[:, :, 0]
        d, n_slots = vectors.shape
        n_query, n_probe = cell_start.shape
        assert query.shape == (d, n_query)
        assert vectors.dtype == query.dtype == torch.float32
        _check_lists(n_slots, is_empty, cell_start, cell_size, n_probe_list)
        assert distance in ("euclidean", "cosine", "inner")
        threshold = _checked_threshold(threshold, n_query)
        query = query.contiguous()
        require_gpu(vectors, query, is_empty, cell_start, cell_size, n_probe_list, _tensor_or_none(threshold))
        device = vectors.device
        inputs = (ptr(vectors), ptr(query), ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list))

        def passes():
            split = self._n_split(n_query, device, slots_hint) if n_split is None else n_split
            self.last_n_split = split
            n_seg = load().tpq_ivfflat_range_segments(n_query, split)
            assert n_seg == n_query * split * 8, (n_query, split)
            shape = (n_slots, d, n_query, n_probe, metric_code(distance), split)
            return (n_seg,
                    lambda thr, counts: call("tpq_ivfflat_range_count", device, *inputs, thr, counts, *shape),
                    lambda thr, *out: call("tpq_ivfflat_range_fill", device, *inputs, thr, *out, *shape))
        return _range_two_pass(n_query, device, threshold, passes)


class IVFPQRangeHip:
    """Range search over the lists of IVFPQIndex (tpq_ivfpq_range_count / _fill and their residual forms,
    csrc/scan_range.hip): every candidate of IVFPQTopkHip whose value is >= the query's threshold, in scan order, the
    value being that of the exact reference-layout scan; the semantics are defined in include/torchpq_amd.h.  The scan
    reads CellContainer._storage itself: there is no scan-layout route."""

    def __init__(self, m=8):
        assert m % 4 == 0
        self.m = m
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last plain call

    _n_split = IVFPQTopkHip._n_split

    def _check_lists(self, data, is_empty, cell_start, cell_size, n_probe_list):
        n_data = data.shape[1]
        n_query, n_probe = cell_start.shape
        assert data.shape == (self.m // 4, n_data, 4) and data.dtype == torch.uint8
        _check_lists(n_data, is_empty, cell_start, cell_size, n_probe_list)
        return n_data, n_query, n_probe

    def _check_fused(self, query, codebook, n_query):
        """(query, codebook, ds) of a table built in the workgroup"""
        m, ds, kk = codebook.shape
        assert m == self.m and kk == 256 and query.shape == (m * ds, n_query)
        assert query.dtype == codebook.dtype == torch.float32
        return query.contiguous(), codebook.contiguous(), ds

    def __call__(self, data, cell_start, cell_size, n_probe_list, threshold, precomputed=None, query=None,
                 codebook=None, distance="euclidean", is_empty=None, n_split=None, slots_hint=None):
        """Plain PQ.
          data: [m // 4, n_data, 4] uint8 (CellContainer._storage)
          precomputed: [m, n_query, 256] float32 (AdcLutHip), or None with query [d, n_query] and codebook
                       [m, ds, 256] float32, from which the workgroup builds the same table (`distance` as AdcLutHip)
          cell_start / cell_size: [n_query, max_n_probe] int64; n_probe_list: [n_query] int64
          threshold: a Python float, or [n_query] float32 -- one per query
          is_empty: [n_data] uint8, or None when no slot inside a cell is a tombstone
        returns (lims [n_query + 1] int64, values [total] float32, address [total] int64): the hits of query q are
        values[lims[q]:lims[q+1]] / address[lims[q]:lims[q+1]], probe rank ascending, then address ascending.
        Synchronises once: the number of hits sizes the outputs.
        """
        n_data, n_query, n_probe = self._check_lists(data, is_empty, cell_start, cell_size, n_probe_list)
        ds = 0
        if precomputed is not None:
            assert precomputed.shape == (self.m, n_query, 256) and precomputed.dtype == torch.float32
            precomputed, query, codebook = precomputed.contiguous(), None, None
        else:
            assert query is not None and codebook is not None
            query, codebook, ds = self._check_fused(query, codebook, n_query)
        assert distance in ("euclidean", "cosine", "inner")
        threshold = _checked_threshold(threshold, n_query)
        require_gpu(data, precomputed, query, codebook, is_empty, cell_start, cell_size, n_probe_list,
                    _tensor_or_none(threshold))
        device = data.device
        inputs = (ptr(data), ptr(precomputed), ptr(query), ptr(codebook), ds, metric_code(distance), ptr(is_empty),
                  ptr(cell_start), ptr(cell_size), ptr(n_probe_list))

        def passes():
            split = self._n_split(n_query, device, slots_hint) if n_split is None else n_split
            self.last_n_split = split
            n_seg = load().tpq_ivfpq_range_segments(n_query, split)
            assert n_seg == n_query * split * 8, (n_query, split)
            shape = (n_data, n_query, n_probe, self.m, split)
            return (n_seg,
                    lambda thr, counts: call("tpq_ivfpq_range_count", device, *inputs, thr, counts, *shape),
                    lambda thr, *out: call("tpq_ivfpq_range_fill", device, *inputs, thr, *out, *shape))
        return _range_two_pass(n_query, device, threshold, passes)

    def residual(self, data, base_sims, cell_start, cell_size, n_probe_list, threshold, part1=None, part2=None,
                 cells=None, full=None, query=None, codebook=None, is_empty=None):
        """Residual PQ: the value of IVFPQTopkHip.topk_residual_precomputed / topk_residual.
          base_sims: [n_query, max_n_probe] float32
          either full [n_query, max_n_probe, m, 256] float32 -- one table per (query, probe) --
          or part2 [n_cells, m, 256] float32 and cells [n_query, max_n_probe] int64 with part1 [n_query, m, 256]
          float32 (ResidualPart1Hip) or, instead of part1, query [d, n_query] and codebook [m, ds, 256] float32, from
          which the workgroup builds it
          everything else, and the result, as __call__; one workgroup per (query, probe): there is no n_split
        """
        n_data, n_query, n_probe = self._check_lists(data, is_empty, cell_start, cell_size, n_probe_list)
        assert base_sims.shape == (n_query, n_probe) and base_sims.dtype == torch.float32
        base_sims = base_sims.contiguous()
        ds = 0
        if full is not None:
            assert full.shape == (n_query, n_probe, self.m, 256) and full.dtype == torch.float32
            full, part1, part2, cells, query, codebook = full.contiguous(), None, None, None, None, None
        else:
            assert part2 is not None and cells is not None
            assert part2.shape[1:] == (self.m, 256) and part2.dtype == torch.float32
            assert cells.shape == (n_query, n_probe) and cells.dtype == torch.int64
            part2, cells = part2.contiguous(), cells.contiguous()
            if part1 is not None:
                assert part1.shape == (n_query, self.m, 256) and part1.dtype == torch.float32
                part1, query, codebook = part1.contiguous(), None, None
            else:
                assert query is not None and codebook is not None
                query, codebook, ds = self._check_fused(query, codebook, n_query)
        threshold = _checked_threshold(threshold, n_query)
        require_gpu(data, part1, query, codebook, part2, full, cells, base_sims, is_empty, cell_start, cell_size,
                    n_probe_list, _tensor_or_none(threshold))
        device = data.device
        inputs = (ptr(data), ptr(part1), ptr(query), ptr(codebook), ds, ptr(part2), ptr(full), ptr(cells),
                  ptr(base_sims), ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list))

        def passes():
            n_seg = load().tpq_ivfpq_range_residual_segments(n_query, n_probe)
            assert n_seg == n_query * n_probe * 8, (n_query, n_probe)
            shape = (n_data, n_query, n_probe, self.m)
            return (n_seg,
                    lambda thr, counts: call("tpq_ivfpq_range_residual_count", device, *inputs, thr, counts, *shape),
                    lambda thr, *out: call("tpq_ivfpq_range_residual_fill", device, *inputs, thr, *out, *shape))
        return _range_two_pass(n_query, device, threshold, passes)


class SlotFilterBuildHip:
    """One row of filter bits from slot addresses (tpq_slot_filter_build, csrc/scan_filtered.hip): bit s & 31 of word
    s >> 5 for every address s in [0, n_slots); other addresses (-1: an unknown id) are ignored."""

    def __call__(self, address, bits, n_slots):
        """address: [n] int64; bits: a zeroed (or to be extended) row, [>= ceil(n_slots / 32)] int32; in place"""
        assert address.dim() == 1 and address.dtype == torch.int64
        assert bits.dim() == 1 and bits.dtype == torch.int32 and bits.numel() * 32 >= n_slots
        address = address.contiguous()
        require_gpu(address, bits)
        if address.numel() and n_slots:
            call("tpq_slot_filter_build", bits.device, ptr(address), address.numel(), ptr(bits), int(n_slots))
        return bits


class IVFPQFilteredTopkHip:
    """Filtered top-k over the lists of IVFPQIndex (tpq_ivfpq_scan_filtered_topk / _residual_topk,
    csrc/scan_filtered.hip): the k best candidates of IVFPQRangeHip whose slot is allowed by the query's row of filter
    bits, by (value descending, address ascending), the value being that of the exact reference-layout scan; the
    semantics are defined in include/torchpq_amd.h.  The scan reads CellContainer._storage itself: there is no
    scan-layout route."""

    def __init__(self, m=8):
        assert m % 4 == 0
        self.m = m
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last plain call

    _n_split = IVFPQTopkHip._n_split
    _check_lists = IVFPQRangeHip._check_lists
    _check_fused = IVFPQRangeHip._check_fused

    @staticmethod
    def _check_filter(filter_bits, filter_of_query, n_data, n_query):
        """filter_bits [n_filters, stride] int32, stride >= ceil(n_data / 32); filter_of_query [n_query] int32 or None"""
        assert filter_bits.dim() == 2 and filter_bits.dtype == torch.int32 and filter_bits.shape[0] >= 1
        assert filter_bits.shape[1] * 32 >= n_data
        if filter_of_query is not None:
            assert filter_of_query.shape == (n_query,) and filter_of_query.dtype == torch.int32
            filter_of_query = filter_of_query.contiguous()
        return filter_of_query

    def __call__(self, data, cell_start, cell_size, n_probe_list, k, filter_bits, filter_of_query=None,
                 precomputed=None, query=None, codebook=None, distance="euclidean", is_empty=None, address2id=None,
                 n_split=None, slots_hint=None):
        """Plain PQ.
          data, cell_start, cell_size, n_probe_list, precomputed or (query, codebook, distance), is_empty: as
          IVFPQRangeHip
          filter_bits: [n_filters, stride] int32, bit s & 31 of word s >> 5 of a row: slot s is allowed
          filter_of_query: [n_query] int32, the row of every query (outside [0, n_filters): no candidate); None: row 0
          address2id: optional [n_data] int64; when given a third tensor (ids) is returned
        returns (values [n_query, k] descending, address [n_query, k][, ids]); unfilled = (-inf, -1[, -1])
        """
        n_data, n_query, n_probe = self._check_lists(data, is_empty, cell_start, cell_size, n_probe_list)
        filter_of_query = self._check_filter(filter_bits, filter_of_query, n_data, n_query)
        ds = 0
        if precomputed is not None:
            assert precomputed.shape == (self.m, n_query, 256) and precomputed.dtype == torch.float32
            precomputed, query, codebook = precomputed.contiguous(), None, None
        else:
            assert query is not None and codebook is not None
            query, codebook, ds = self._check_fused(query, codebook, n_query)
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= 1024
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        require_gpu(data, precomputed, query, codebook, is_empty, cell_start, cell_size, n_probe_list, filter_bits,
                    filter_of_query, address2id)
        device = data.device
        values, address, ids = alloc_topk(n_query, k, device, address2id)
        if n_query == 0:
            return topk_result(values, address, ids)
        n_split, ws, ws_bytes = _split_and_workspace(self, load().tpq_ivfpq_scan_filtered_workspace_bytes, n_query, k,
                                                     n_split, slots_hint, device)
        call("tpq_ivfpq_scan_filtered_topk", device,
             ptr(data), ptr(precomputed), ptr(query), ptr(codebook), ds, metric_code(distance), ptr(is_empty),
             ptr(cell_start), ptr(cell_size), ptr(n_probe_list), ptr(filter_bits), ptr(filter_of_query),
             filter_bits.shape[0], filter_bits.shape[1], ptr(values), ptr(address), ptr(address2id), ptr(ids), n_data,
             n_query, n_probe, self.m, k, n_split, ptr(ws), ws_bytes)
        return topk_result(values, address, ids)

    def residual(self, data, base_sims, cell_start, cell_size, n_probe_list, k, filter_bits, filter_of_query=None,
                 part1=None, part2=None, cells=None, full=None, query=None, codebook=None, is_empty=None,
                 address2id=None):
        """Residual PQ: base_sims and the tables as IVFPQRangeHip.residual, everything else, and the result, as
        __call__; one workgroup per query: there is no n_split"""
        n_data, n_query, n_probe = self._check_lists(data, is_empty, cell_start, cell_size, n_probe_list)
        filter_of_query = self._check_filter(filter_bits, filter_of_query, n_data, n_query)
        assert base_sims.shape == (n_query, n_probe) and base_sims.dtype == torch.float32
        base_sims = base_sims.contiguous()
        ds = 0
        if full is not None:
            assert full.shape == (n_query, n_probe, self.m, 256) and full.dtype == torch.float32
            full, part1, part2, cells, query, codebook = full.contiguous(), None, None, None, None, None
        else:
            assert part2 is not None and cells is not None
            assert part2.shape[1:] == (self.m, 256) and part2.dtype == torch.float32
            assert cells.shape == (n_query, n_probe) and cells.dtype == torch.int64
            part2, cells = part2.contiguous(), cells.contiguous()
            if part1 is not None:
                assert part1.shape == (n_query, self.m, 256) and part1.dtype == torch.float32
                part1, query, codebook = part1.contiguous(), None, None
            else:
                assert query is not None and codebook is not None
                query, codebook, ds = self._check_fused(query, codebook, n_query)
        assert 0 < k <= 1024
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        require_gpu(data, part1, query, codebook, part2, full, cells, base_sims, is_empty, cell_start, cell_size,
                    n_probe_list, filter_bits, filter_of_query, address2id)
        device = data.device
        values, address, ids = alloc_topk(n_query, k, device, address2id)
        if n_query:
            call("tpq_ivfpq_scan_filtered_residual_topk", device,
                 ptr(data), ptr(part1), ptr(query), ptr(codebook), ds, ptr(part2), ptr(full), ptr(cells),
                 ptr(base_sims), ptr(is_empty), ptr(cell_start), ptr(cell_size), ptr(n_probe_list), ptr(filter_bits),
                 ptr(filter_of_query), filter_bits.shape[0], filter_bits.shape[1], ptr(values), ptr(address),
                 ptr(address2id), ptr(ids), n_data, n_query, n_probe, self.m, k)
        return topk_result(values, address, ids)


class IVFPQ4FilteredTopkHip:
    """Filtered top-k over the lists of IVFPQ4Index (tpq_ivfpq4_scan_filtered_topk / _residual_topk,
    csrc/scan_pq4_filtered.hip): the result of IVFPQ4TopkHip / IVFPQ4ResidualTopkHip among the slots the query's row of
    filter bits allows, bit for bit what those give with `is_empty | ~allowed_row` as the tombstone mask; the semantics
    are defined in include/torchpq_amd.h."""

    def __init__(self, m=8):
        assert m % 8 == 0 and 8 <= m <= 256, "4-bit codes are stored 8 sub-quantizers per word; 8 <= m <= 256"
        self.m = m
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last call

    _n_split = IVFFlatTopkHip._n_split

    def _scan(self, symbol, codes, query, codebook, residual, cell_start, cell_size, n_probe_list, k, filter_bits,
              filter_of_query, is_empty, distance, n_split, slots_hint):
        """both calls; `residual` is () or (centroids, cells)"""
        n_slots = codes.shape[1]
        m, ds, kk = codebook.shape
        n_query, n_probe = cell_start.shape
        assert m == self.m and kk == 16 and ds >= 1
        assert codes.shape == (m // 8, n_slots, 4) and codes.dtype == torch.uint8 and codes.is_contiguous()
        assert query.shape == (m * ds, n_query)
        assert query.dtype == codebook.dtype == torch.float32
        _check_lists(n_slots, is_empty, cell_start, cell_size, n_probe_list)
        filter_of_query = IVFPQFilteredTopkHip._check_filter(filter_bits, filter_of_query, n_slots, n_query)
        assert filter_bits.is_contiguous()
        tables = ()
        if residual:
            centroids, cells = residual
            assert centroids.dtype == torch.float32
            assert centroids.dim() == 2 and centroids.shape[0] >= 1 and centroids.shape[1] == m * ds
            assert cells.shape == (n_query, n_probe) and cells.dtype == torch.int64
            centroids, cells = centroids.contiguous(), cells.contiguous()
            tables = (ptr(centroids), ptr(cells), centroids.shape[0])
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= 1024
        query = query.contiguous()
        codebook = codebook.contiguous()
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        require_gpu(codes, query, codebook, *residual, is_empty, cell_start, cell_size, n_probe_list, filter_bits,
                    filter_of_query)
        device = codes.device
        values, address = alloc_pair(n_query, k, device)
        if n_query == 0:
            return values, address
        n_split, ws, ws_bytes = _split_and_workspace(self, load().tpq_ivfpq4_scan_workspace_bytes, n_query, k,
                                                     n_split, slots_hint, device)
        call(symbol, device,
             ptr(codes), ptr(query), ptr(codebook), *tables, ptr(is_empty), ptr(cell_start), ptr(cell_size),
             ptr(n_probe_list), ptr(filter_bits), ptr(filter_of_query), filter_bits.shape[0], filter_bits.shape[1],
             ptr(values), ptr(address), n_slots, m, ds, n_query, n_probe, k, metric_code(distance), n_split, ptr(ws),
             ws_bytes)
        return values, address

    def __call__(self, codes, query, codebook, cell_start, cell_size, n_probe_list, k, filter_bits,
                 filter_of_query=None, is_empty=None, distance="euclidean", n_split=None, slots_hint=None):
        """Plain codes.
          codes, query, codebook, cell_start, cell_size, n_probe_list, is_empty: as IVFPQ4TopkHip
          filter_bits: [n_filters, stride] int32, bit s & 31 of word s >> 5 of a row: slot s is allowed
          filter_of_query: [n_query] int32, the row of every query (outside [0, n_filters): no candidate); None: row 0
        returns (values [n_query, k] descending, address [n_query, k]); unfilled = (-inf, -1)
        """
        return self._scan("tpq_ivfpq4_scan_filtered_topk", codes, query, codebook, (), cell_start, cell_size,
                          n_probe_list, k, filter_bits, filter_of_query, is_empty, distance, n_split, slots_hint)

    def residual(self, codes, query, codebook, centroids, cells, cell_start, cell_size, n_probe_list, k, filter_bits,
                 filter_of_query=None, is_empty=None, distance="euclidean", n_split=None, slots_hint=None):
        """Residual codes: centroids [n_cells, d] and cells [n_query, max_n_probe] as IVFPQ4ResidualTopkHip, everything
        else, and the result, as __call__"""
        return self._scan("tpq_ivfpq4_scan_filtered_residual_topk", codes, query, codebook, (centroids, cells),
                          cell_start, cell_size, n_probe_list, k, filter_bits, filter_of_query, is_empty, distance,
                          n_split, slots_hint)


class IVFPQ4RangeHip:
    """Range search over the lists of IVFPQ4Index (tpq_ivfpq4_range_count / _fill and their residual forms,
    csrc/scan_pq4_range.hip): every candidate of IVFPQ4TopkHip / IVFPQ4ResidualTopkHip whose value is >= the query's
    threshold, in scan order, optionally among the slots the query's row of filter bits allows; a hit carries the bits
    those scans return for the slot; the semantics are defined in include/torchpq_amd.h."""

    def __init__(self, m=8):
        assert m % 8 == 0 and 8 <= m <= 256, "4-bit codes are stored 8 sub-quantizers per word; 8 <= m <= 256"
        self.m = m
        self.n_cus = None
        self.last_n_split = None   # diagnostics / tests: workgroups per query of the last plain call

    _n_split = IVFFlatTopkHip._n_split

    def _inputs(self, codes, query, codebook, residual, cell_start, cell_size, n_probe_list, threshold, filter_bits,
                filter_of_query, is_empty, distance):
        """the checks both calls share; `residual` is () or (centroids, cells) -> (the count / fill arguments in
        front of the threshold, the checked threshold, (n_slots, m, ds, n_query, n_probe, metric), device)"""
        n_slots = codes.shape[1]
        m, ds, kk = codebook.shape
        n_query, n_probe = cell_start.shape
        assert m == self.m and kk == 16 and ds >= 1
        assert codes.shape == (m // 8, n_slots, 4) and codes.dtype == torch.uint8 and codes.is_contiguous()
        assert query.shape == (m * ds, n_query)
        assert query.dtype == codebook.dtype == torch.float32
        _check_lists(n_slots, is_empty, cell_start, cell_size, n_probe_list)
        flt = (None, None, 0, 0)
        if filter_bits is not None:
            filter_of_query = IVFPQFilteredTopkHip._check_filter(filter_bits, filter_of_query, n_slots, n_query)
            assert filter_bits.is_contiguous()
            flt = (ptr(filter_bits), ptr(filter_of_query), filter_bits.shape[0], filter_bits.shape[1])
        else:
            assert filter_of_query is None, "filter_of_query without filter_bits"
        tables = ()
        if residual:
            centroids, cells = residual
            assert centroids.dtype == torch.float32
            assert centroids.dim() == 2 and centroids.shape[0] >= 1 and centroids.shape[1] == m * ds
            assert cells.shape == (n_query, n_probe) and cells.dtype == torch.int64
            centroids, cells = centroids.contiguous(), cells.contiguous()
            tables = (ptr(centroids), ptr(cells), centroids.shape[0])
            residual = (centroids, cells)
        assert distance in ("euclidean", "cosine", "inner")
        threshold = _checked_threshold(threshold, n_query)
        query = query.contiguous()
        codebook = codebook.contiguous()
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        require_gpu(codes, query, codebook, *residual, is_empty, cell_start, cell_size, n_probe_list, filter_bits,
                    filter_of_query, _tensor_or_none(threshold))
        # (the tensors made contiguous above live until the passes have been launched: the closure holds them)
        keep = (query, codebook, residual, cell_start, cell_size, filter_of_query)
        inputs = (ptr(codes), ptr(query), ptr(codebook), *tables, ptr(is_empty), ptr(cell_start), ptr(cell_size),
                  ptr(n_probe_list), *flt)
        return inputs, threshold, (n_slots, m, ds, n_query, n_probe, metric_code(distance)), codes.device, keep

    def __call__(self, codes, query, codebook, cell_start, cell_size, n_probe_list, threshold, filter_bits=None,
                 filter_of_query=None, is_empty=None, distance="euclidean", n_split=None, slots_hint=None):
        """Plain codes.
          codes, query, codebook, cell_start, cell_size, n_probe_list, is_empty: as IVFPQ4TopkHip
          threshold: a Python float, or [n_query] float32 -- one per query
          filter_bits: None, or [n_filters, stride] int32, bit s & 31 of word s >> 5 of a row: slot s is allowed
          filter_of_query: [n_query] int32, the row of every query (outside [0, n_filters): no hit); None: row 0
        returns (lims [n_query + 1] int64, values [total] float32, address [total] int64): the hits of query q are
        values[lims[q]:lims[q+1]] / address[lims[q]:lims[q+1]], probe rank ascending, then address ascending.
        Synchronises once: the number of hits sizes the outputs.
        """
        inputs, threshold, shape, device, keep = self._inputs(
            codes, query, codebook, (), cell_start, cell_size, n_probe_list, threshold, filter_bits, filter_of_query,
            is_empty, distance)
        n_query = shape[3]

        def passes():
            split = self._n_split(n_query, device, slots_hint) if n_split is None else n_split
            self.last_n_split = split
            n_seg = load().tpq_ivfpq4_range_segments(n_query, split)
            assert n_seg == n_query * split * 8, (n_query, split)
            return (n_seg,
                    lambda thr, counts: call("tpq_ivfpq4_range_count", device, *inputs, thr, counts, *shape, split),
                    lambda thr, *out: call("tpq_ivfpq4_range_fill", device, *inputs, thr, *out, *shape, split))
        return _range_two_pass(n_query, device, threshold, passes)

    def residual(self, codes, query, codebook, centroids, cells, cell_start, cell_size, n_probe_list, threshold,
                 filter_bits=None, filter_of_query=None, is_empty=None, distance="euclidean"):
        """Residual codes: centroids [n_cells, d] and cells [n_query, max_n_probe] as IVFPQ4ResidualTopkHip, everything
        else, and the result, as __call__; one workgroup per (query, probe): there is no n_split"""
        inputs, threshold, shape, device, keep = self._inputs(
            codes, query, codebook, (centroids, cells), cell_start, cell_size, n_probe_list, threshold, filter_bits,
            filter_of_query, is_empty, distance)
        n_query, n_probe = shape[3], shape[4]

        def passes():
            n_seg = load().tpq_ivfpq4_range_residual_segments(n_query, n_probe)
            assert n_seg == n_query * n_probe * 8, (n_query, n_probe)
            return (n_seg,
                    lambda thr, counts: call("tpq_ivfpq4_range_residual_count", device, *inputs, thr, counts, *shape),
                    lambda thr, *out: call("tpq_ivfpq4_range_residual_fill", device, *inputs, thr, *out, *shape))
        return _range_two_pass(n_query, device, threshold, passes)


# ---- what the range wrappers share --------------------------------------------------------------------------------
def _checked_threshold(threshold, n_query):
    """a range search's threshold: a Python float, or one float32 per query (returned contiguous)"""
    if not torch.is_tensor(threshold):
        return float(threshold)
    assert threshold.shape == (n_query,) and threshold.dtype == torch.float32
    return threshold.contiguous()


def _tensor_or_none(threshold):
    return threshold if torch.is_tensor(threshold) else None


def _range_two_pass(n_query, device, threshold, passes):
    """The driver of a two-pass range search: count -> the caller's prefix sum -> one .item() -> fill.
    `passes()` -- called only for a non-empty batch -- returns (segments, count(thr, counts), fill(thr, offsets,
    values, address)), the two launches taking device pointers; segment s belongs to query s // (segments // n_query).
    Returns (lims [n_query + 1] int64, values [total] float32, address [total] int64)."""
    if n_query == 0:
        return (torch.zeros(1, device=device, dtype=torch.int64),
                torch.empty(0, device=device, dtype=torch.float32),
                torch.empty(0, device=device, dtype=torch.int64))
    if not torch.is_tensor(threshold):
        threshold = torch.full((n_query,), threshold, device=device, dtype=torch.float32)
    n_seg, count, fill = passes()
    counts = torch.empty(n_seg, device=device, dtype=torch.int32)
    count(ptr(threshold), ptr(counts))
    offsets = torch.zeros(n_seg + 1, device=device, dtype=torch.int64)
    offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
    total = int(offsets[-1].item())     # the host sync a variable-size output needs
    values = torch.empty(total, device=device, dtype=torch.float32)
    address = torch.empty(total, device=device, dtype=torch.int64)
    if total:
        fill(ptr(threshold), ptr(offsets), ptr(values), ptr(address))
    return offsets[::n_seg // n_query].contiguous(), values, address
