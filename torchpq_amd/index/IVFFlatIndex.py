"""IVFFlatIndex: coarse quantizer and inverted lists with the vectors stored as they are.

Recall is limited only by `n_probe`, not by a product quantizer.  The container is CellContainer unchanged: a vector
of d floats is stored as code_size = 4 d bytes, row i holding the four bytes of component i, so `_storage` is uint8
[d, capacity, 4] and `_storage.view(torch.float32)` is [d, capacity, 1] -- dimension-major and slot-contiguous, the
layout FlatIndex uses, fully coalesced for the list scan (tpq_ivfflat_scan_topk, csrc/scan_flat.hip), which reads
it in place.  add / expand / remove / tombstones / `_address2id` / state_dict are the container's.

The coarse step is IVFPQIndex's (index/_coarse.py).

Filtered search (search_filtered, range_search_filtered) hands the scan a filter row as its skip mask: IdFilter.masks()
is the row's complement OR-ed with the tombstones, and the masked form of the scan reads a slot's mask byte before any
of its 4 d bytes of vector, so a tile without an allowed slot costs 64 bytes, not 256 d.
"""
import torch

from ..container import CellContainer
from ..kernels import IVFFlatRangeHip, IVFFlatTopkHip
from ._coarse import CoarseProbeMixin
from ._filter import IdFilter, checked_filter_rows, filtered_search_batches, queries_by_row
from ._range import range_search_batches


class IVFFlatIndex(CoarseProbeMixin, CellContainer):
    def __init__(self, d_vector, n_cells=128, initial_size=None, expand_step_size=128, expand_mode="double",
                 distance="euclidean", device="cuda:0", verbose=0):
        assert d_vector >= 1
        assert distance in ("euclidean", "cosine")
        if torch.device(device).type == "cuda":
            assert torch.cuda.is_available(), "cuda is not available"
        super().__init__(code_size=4 * d_vector, n_cells=n_cells, dtype="uint8", device=device,
                         initial_size=initial_size, expand_step_size=expand_step_size,
                         expand_mode=expand_mode, use_inverse_id_mapping=True, contiguous_size=4,
                         verbose=verbose)
        self.d_vector = d_vector
        self.distance = distance
        self.verbose = verbose
        self.use_cublas = True
        self._init_coarse(n_cells, verbose)
        self._flat_topk = IVFFlatTopkHip()
        self._flat_range = IVFFlatRangeHip()
        self.to(device)

    def _after_load_state_dict(self):
        self.to(self.device)
        super()._after_load_state_dict()

    # ---- the byte layout -----------------------------------------------------------------------------
    @staticmethod
    def vectors_to_codes(x):
        """[d, n] float32 -> the container's code rows [4 d, n] uint8: row 4 i + b is byte b of component i"""
        d, n = x.shape
        return x.contiguous().view(torch.uint8).reshape(d, n, 4).transpose(1, 2).reshape(4 * d, n)

    @staticmethod
    def codes_to_vectors(codes):
        """[4 d, n] uint8 -> [d, n] float32 (the inverse of vectors_to_codes)"""
        d4, n = codes.shape
        return codes.reshape(d4 // 4, 4, n).transpose(1, 2).contiguous().view(torch.float32).reshape(d4 // 4, n)

    def _vectors(self):
        """the stored vectors as the scan reads them, [d_vector, capacity] float32 (a view of `_storage`)"""
        return self._storage.view(torch.float32)[:, :, 0]

    # ---- train / add -----------------------------------------------------------------------------------
    def train(self, x, force_retrain=False):
        """x [d_vector, n_data] f32: the coarse k-means (n_cells) only."""
        if self.vq_codec.is_trained and not force_retrain:
            self.print_message("index is already trained", 1)
            return
        x = self._prepare(x)
        self.print_message("start training VQ codec...", 1)
        self.vq_codec.train(x)
        self.print_message("index is trained successfully!", 1)

    def add(self, x, ids=None, return_address=False):
        """x [d_vector, n] f32 (stored normalised for "cosine"), optional ids [n] int64 (default arange + max_id
        + 1); returns ids (and the slot addresses if return_address)."""
        assert x.dtype == torch.float32
        x = self._prepare(x)
        assert self.vq_codec.is_trained, "index is not trained"
        assigned_cells = self.vq_codec.encode(x)
        return super().add(self.vectors_to_codes(x), cells=assigned_cells, ids=ids, return_address=return_address)

    def reconstruct(self, ids=None, address=None):
        """the stored vectors [d_vector, n] f32 of `ids` (or of slot addresses): bit for bit what add() stored
        (the normalised vector for "cosine"); zero columns for unknown ids / invalid addresses"""
        if ids is not None:
            address = self.get_address_by_id(ids.to(self.device))
        elif address is None:
            raise RuntimeError("Need either ids or address")
        address = address.to(self.device)
        live = (address >= 0) & (address < self.capacity)
        live &= self._is_empty[torch.where(live, address, torch.zeros_like(address))] == 0
        address = torch.where(live, address, torch.full_like(address, -1))
        return self.codes_to_vectors(self.get_data_by_address(address))

    # ---- search ----------------------------------------------------------------------------------------
    def search_cells(self, x, cells, base_sims=None, n_probe_list=None, k=1, return_address=False, _extents=None):
        """Scan the given cells [n_query, n_probe] for each query; (values, ids[, address]).
        (`base_sims` is accepted for IVFPQIndex's signature and unused; `_extents`: the cells' (start, size) when
        the coarse step already gathered them.)"""
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        _extents)
        vals, address = self._flat_topk(
            self._vectors(), x, cell_start.contiguous(), cell_size.contiguous(), n_probe_list, k,
            is_empty=is_empty, distance=self.distance, slots_hint=slots_hint)
        ids = self.get_id_by_address(address)
        return (vals, ids, address) if return_address else (vals, ids)

    def graphed_search(self, n_query, k=1):
        raise NotImplementedError("GraphedSearch captures IVFPQIndex.search only")

    def search(self, x, k=1, return_address=False):
        """x [d_vector, n_query] f32 -> (values f32 [n_query, k] descending, ids int64 [n_query, k][, address]);
        values are -squared-L2 (euclidean) or the cosine similarity to the stored vectors; (-inf, -1) pads."""
        x = self._prepare(x)
        assert 0 < k <= 1024
        assert self.vq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        vals, ids, address = self._search_batches(x, lambda xb, sims, cells, n_probe_list, extents: self.search_cells(
            x=xb, cells=cells, base_sims=sims, n_probe_list=n_probe_list, k=k, return_address=True,
            _extents=extents))
        return (vals, ids, address) if return_address else (vals, ids)

    # ---- filtered search -------------------------------------------------------------------------------
    def id_filter(self, ids):
        """ids: an int64 tensor -- one set of allowed ids -- or a sequence of them, one filter row each -> IdFilter,
        what search_filtered and range_search_filtered take.  Ids the index does not hold are ignored; the filter
        follows later add / remove."""
        return IdFilter(self, ids)

    def search_cells_filtered(self, x, cells, flt, filter_of_query=None, n_probe_list=None, k=1,
                              return_address=False, _extents=None):
        """The k best live vectors of the given cells [n_query, n_probe] among the ids `flt` allows; (values, ids[,
        address]), (-inf, -1) where fewer exist.  `filter_of_query`: an int tensor [n_query], the row of `flt` every
        query uses (None: row 0); a row outside [0, n_filters) allows nothing.  The scan takes one mask per launch:
        the queries are grouped by row and every group is one launch with its row of `flt.masks()`, so a batch with
        many distinct rows pays one launch per row.  When `filter_of_query` is given and the filter has more than one
        row, the rows are read back to form the groups -- one host synchronisation per call; with one row, or without
        `filter_of_query`, there is none.  (`_extents` as in search_cells.)"""
        assert isinstance(flt, IdFilter), "flt is what index.id_filter(ids) returns"
        n_probe_list, cell_start, cell_size, slots_hint, _ = self._scan_preamble(x, cells, n_probe_list, _extents)
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        masks = flt.masks(self)
        n_query = x.shape[1]
        scan = lambda row, xg, cs, sz, npl: self._flat_topk(
            self._vectors(), xg, cs, sz, npl, k, is_empty=masks[row], distance=self.distance, slots_hint=slots_hint)
        if filter_of_query is None or flt.n_filters == 1:
            vals, address = scan(0, x, cell_start, cell_size, n_probe_list)
            if filter_of_query is not None:      # a row other than 0 allows nothing
                other = (filter_of_query != 0)[:, None]
                vals = vals.masked_fill(other, float("-inf"))
                address = address.masked_fill(other, -1)
        else:
            vals = torch.full((n_query, k), float("-inf"), device=self.device, dtype=torch.float32)
            address = torch.full((n_query, k), -1, device=self.device, dtype=torch.int64)
            for row, queries in queries_by_row(filter_of_query, n_query, flt.n_filters, self.device):
                if queries is None:
                    vals, address = scan(row, x, cell_start, cell_size, n_probe_list)
                else:
                    v, a = scan(row, x[:, queries], cell_start[queries], cell_size[queries], n_probe_list[queries])
                    vals[queries] = v
                    address[queries] = a
        ids = self.get_id_by_address(address) if address.numel() else torch.empty_like(address)
        return (vals, ids, address) if return_address else (vals, ids)

    def search_filtered(self, x, k, flt, filter_of_query=None):
        """x [d_vector, n_query] f32, flt = index.id_filter(ids) -> (values f32 [n_query, k] descending, ids int64
        [n_query, k]): the k best stored vectors of the query's probed cells (`n_probe`, as in search) AMONG the ids the
        filter allows, padded with (-inf, -1) where fewer exist.  `filter_of_query`: an int tensor [n_query] choosing
        the filter's row per query (a filter made from a sequence of id sets); the default is row 0 for every query.
        A result carries the value search returns for the same vector; equal values come by ascending slot address.
        One launch per distinct row of a batch, and one host synchronisation per batch of `max_query_batch` queries
        when rows are given and the filter has more than one (search_cells_filtered)."""
        x = self._prepare(x)
        assert 0 < k <= 1024
        assert self.vq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        return filtered_search_batches(
            self, x, flt, filter_of_query, lambda xb, rows, sims, cells, n_probe_list, extents:
            self.search_cells_filtered(xb, cells, flt, filter_of_query=rows, n_probe_list=n_probe_list, k=k,
                                       _extents=extents))

    # ---- range search ----------------------------------------------------------------------------------
    def range_search_cells(self, x, cells, threshold, n_probe_list=None, return_address=False, _extents=None):
        """Every live vector of the given cells [n_query, n_probe] whose value is >= `threshold` (a float, or f32
        [n_query]); (lims, values, ids[, address]) in scan order, see range_search.  (`_extents` as in search_cells.)"""
        return self._range_cells(x, cells, threshold, n_probe_list, return_address, _extents, None, None)

    def range_search_cells_filtered(self, x, cells, threshold, flt, filter_of_query=None, n_probe_list=None,
                                    return_address=False, _extents=None):
        """range_search_cells among the ids `flt` allows; `filter_of_query` chooses the filter's row per query, as in
        search_cells_filtered: one pair of passes per distinct row, the segments put back in query order."""
        assert isinstance(flt, IdFilter), "flt is what index.id_filter(ids) returns"
        return self._range_cells(x, cells, threshold, n_probe_list, return_address, _extents, flt, filter_of_query)

    def _range_cells(self, x, cells, threshold, n_probe_list, return_address, extents, flt, filter_of_query):
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        extents)
        cell_start, cell_size = cell_start.contiguous(), cell_size.contiguous()
        scan = lambda mask, xg, cs, sz, npl, thr: self._flat_range(
            self._vectors(), xg, cs, sz, npl, thr, is_empty=mask, distance=self.distance, slots_hint=slots_hint)
        if flt is None:
            lims, vals, address = scan(is_empty, x, cell_start, cell_size, n_probe_list, threshold)
        else:
            lims, vals, address = self._range_by_row(scan, flt.masks(self), x, cell_start, cell_size, n_probe_list,
                                                     threshold, filter_of_query)
        ids = self.get_id_by_address(address) if address.numel() else torch.empty_like(address)
        return (lims, vals, ids, address) if return_address else (lims, vals, ids)

    def _range_by_row(self, scan, masks, x, cell_start, cell_size, n_probe_list, threshold, filter_of_query):
        """the filtered range search of one batch: a scan per distinct filter row over the queries that use it, the
        segments put back in query order -> (lims, values, address)"""
        n_query = x.shape[1]
        groups = queries_by_row(filter_of_query, n_query, masks.shape[0], self.device)
        if len(groups) == 1 and groups[0][1] is None:
            return scan(masks[groups[0][0]], x, cell_start, cell_size, n_probe_list, threshold)
        counts = torch.zeros(n_query, device=self.device, dtype=torch.int64)
        parts = []
        for row, queries in groups:
            thr = threshold[queries] if torch.is_tensor(threshold) else threshold
            lg, vg, ag = scan(masks[row], x[:, queries], cell_start[queries], cell_size[queries],
                              n_probe_list[queries], thr)
            counts[queries] = lg.diff()
            parts.append((queries, lg, vg, ag))
        lims = torch.zeros(n_query + 1, device=self.device, dtype=torch.int64)
        lims[1:] = counts.cumsum(0)
        total = sum(vg.numel() for _, _, vg, _ in parts)
        vals = torch.empty(total, device=self.device, dtype=torch.float32)
        address = torch.empty(total, device=self.device, dtype=torch.int64)
        for queries, lg, vg, ag in parts:
            if not vg.numel():
                continue
            # hit i of the group belongs to its query j: it goes where that query's segment starts, plus i - lg[j]
            j = torch.repeat_interleave(torch.arange(queries.numel(), device=self.device), lg.diff(),
                                        output_size=vg.numel())
            dest = lims[queries][j] + torch.arange(vg.numel(), device=self.device) - lg[j]
            vals[dest] = vg
            address[dest] = ag
        return lims, vals, address

    def range_search(self, x, threshold, return_address=False, sort=False):
        """x [d_vector, n_query] f32, threshold a float or f32 [n_query] -> (lims int64 [n_query + 1], values f32
        [total], ids int64 [total][, address]): the hits of query q are values[lims[q]:lims[q+1]] and
        ids[lims[q]:lims[q+1]] -- every stored vector of the query's probed cells (`n_probe`, as in search) whose value
        is >= threshold.  `threshold` is in the index's value space, the one search returns: -squared-L2 for
        "euclidean" (all vectors within distance r: threshold = -r * r), the cosine similarity for "cosine".
        Hits come in scan order (probe rank, then slot address); sort=True orders each query's hits by value
        descending, equal values by address ascending.  Synchronises once per batch of `max_query_batch` queries:
        the number of hits sizes the outputs."""
        x = self._prepare(x)
        assert self.vq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        return range_search_batches(
            self, x, threshold, lambda xb, thr, sims, cells, n_probe_list, extents: self.range_search_cells(
                xb, cells, thr, n_probe_list, return_address=True, _extents=extents), return_address, sort)

    def range_search_filtered(self, x, threshold, flt, filter_of_query=None, return_address=False, sort=False):
        """range_search among the ids a filter allows: flt = index.id_filter(ids), `filter_of_query` (an int tensor
        [n_query]) chooses its row per query as in search_filtered (default: row 0; a row outside [0, n_filters) has
        no hit).  The same values, order and outputs as range_search.  One pair of passes, and one synchronisation, per
        distinct row of a batch of `max_query_batch` queries."""
        x = self._prepare(x)
        assert self.vq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        rows = checked_filter_rows(self, x, flt, filter_of_query)
        return range_search_batches(
            self, x, threshold, lambda xb, thr, rows_b, sims, cells, n_probe_list, extents:
            self.range_search_cells_filtered(xb, cells, thr, flt, rows_b, n_probe_list, return_address=True,
                                             _extents=extents), return_address, sort, alongside=(rows,))
