"""IVFPQ4Index: coarse quantizer and inverted lists of 4-bit product-quantized codes.

Sixteen centroids per sub-quantizer, two sub-quantizers per byte: half the code bytes of IVFPQIndex at a given
n_subvectors.  The container is CellContainer unchanged with code_size = n_subvectors // 2 and contiguous_size = 4, so
`_storage` is uint8 [n_subvectors // 8, capacity, 4]; the list scan (tpq_ivfpq4_scan_topk, csrc/scan_pq4.hip) reads it
in place -- a 16-entry table row has no LDS bank conflicts whatever the codes are, so there is no scan-layout copy --
and builds the query's table (n_subvectors x 16 floats) inside the scan workgroup.  add / expand / remove / tombstones /
`_address2id` / state_dict are the container's.  `search_filtered` (tpq_ivfpq4_scan_filtered_topk / _residual_topk,
csrc/scan_pq4_filtered.hip) gives the k best among an allowed id set, for both `pq_use_residual` settings, on the bit
rows of `id_filter`.  `range_search` / `range_search_filtered` (tpq_ivfpq4_range_count / _fill and their residual forms,
csrc/scan_pq4_range.hip) give every stored code of the probed cells whose value reaches a threshold -- the value `search`
returns for it, bit for bit -- on a two-pass scan of the same lists, optionally among the ids a filter allows.  No
captured graph.

`pq_use_residual=True` (semantically IVFPQIndex's): the PQ is learnt on, and a slot holds the code of,
x - centroid(cell(x)); `encode` returns (pq_code, vq_code) and `decode` takes that pair and returns centroid + codeword.
The list scan is then tpq_ivfpq4_scan_residual_topk: the scan workgroup rebuilds its n_subvectors x 16 table for every
probe from the query, the codebook and the probed cell's centroid, so a value is the metric between the query and exactly
what `decode` returns, and no table exists in memory.  The only derived state is a cell-major copy of the coarse codebook
([n_cells, d_vector] floats), cached, rebuilt when the coarse codebook changes and not part of the state_dict.  For
"cosine" the residuals are those of the normalised vectors and a value is the inner product with the reconstruction.

The coarse step is IVFPQIndex's (index/_coarse.py).
"""
import torch

from .. import util
from ..codec import PQ4Codec
from ..container import CellContainer
from ..kernels import IVFPQ4FilteredTopkHip, IVFPQ4RangeHip, IVFPQ4ResidualTopkHip, IVFPQ4TopkHip
from ._coarse import CoarseProbeMixin
from ._filter import IdFilter, checked_filter_rows, filtered_search_batches
from ._range import range_search_batches


class IVFPQ4Index(CoarseProbeMixin, CellContainer):
    def __init__(self, d_vector, n_subvectors=8, n_cells=128, initial_size=None, expand_step_size=128,
                 expand_mode="double", distance="euclidean", device="cuda:0", pq_use_residual=False,
                 verbose=0):
        if torch.device(device).type == "cuda":
            assert torch.cuda.is_available(), "cuda is not available"
        assert d_vector % n_subvectors == 0
        assert n_subvectors % 8 == 0, "codes are stored 8 sub-quantizers per word (two per byte, contiguous_size=4)"
        assert 8 <= n_subvectors <= 256
        assert distance in ("euclidean", "cosine")
        super().__init__(code_size=n_subvectors // 2, n_cells=n_cells, dtype="uint8", device=device,
                         initial_size=initial_size, expand_step_size=expand_step_size,
                         expand_mode=expand_mode, use_inverse_id_mapping=True, contiguous_size=4,
                         verbose=verbose)
        self.d_vector = d_vector
        self.n_subvectors = n_subvectors
        self.d_subvector = d_vector // n_subvectors
        self.distance = distance
        self.verbose = verbose
        self.pq_use_residual = bool(pq_use_residual)
        self.use_cublas = True
        self._init_coarse(n_cells, verbose)
        self.pq_codec = PQ4Codec(d_vector=d_vector, n_subvectors=n_subvectors, distance=distance, verbose=verbose)
        self._pq4_topk = (IVFPQ4ResidualTopkHip if self.pq_use_residual else IVFPQ4TopkHip)(m=n_subvectors)
        self._pq4_filtered = IVFPQ4FilteredTopkHip(m=n_subvectors)
        self._pq4_range = IVFPQ4RangeHip(m=n_subvectors)
        self.to(device)

    # ---- knobs (as IVFPQIndex) -------------------------------------------------------------------------
    def _codec_knob(codec, attr, typed):
        def getter(self):
            return getattr(getattr(self, codec).kmeans, attr)

        def setter(self, value):
            if typed:
                assert type(value) is int
                assert value > 0
            assert not getattr(self, codec).is_trained, f"{codec} is already trained"
            setattr(getattr(self, codec).kmeans, attr, value)
        return property(getter, setter)

    vq_codec_max_iter = _codec_knob("vq_codec", "max_iter", True)
    vq_codec_n_redo = _codec_knob("vq_codec", "n_redo", True)
    vq_codec_tolerance = _codec_knob("vq_codec", "tol", False)
    pq_codec_max_iter = _codec_knob("pq_codec", "max_iter", True)
    pq_codec_n_redo = _codec_knob("pq_codec", "n_redo", True)
    pq_codec_tolerance = _codec_knob("pq_codec", "tol", False)
    del _codec_knob

    def _after_load_state_dict(self):
        self.to(self.device)
        super()._after_load_state_dict()

    # ---- train / encode / add --------------------------------------------------------------------------
    def train(self, x, force_retrain=False):
        """x [d_vector, n_data] f32: coarse k-means (n_cells) then 16-centroid PQ codebooks (of the residuals
        x - centroid(cell(x)) with pq_use_residual; the caller's tensor is left as it is)."""
        if self.vq_codec.is_trained and self.pq_codec.is_trained and not force_retrain:
            self.print_message("index is already trained", 1)
            return
        x = self._prepare(x)
        self.print_message("start training VQ codec...", 1)
        self.vq_codec.train(x)
        self.print_message("start training PQ codec...", 1)
        self.pq_codec.train(self._residual(x, self.vq_codec.encode(x)) if self.pq_use_residual else x)
        self.print_message("index is trained successfully!", 1)

    def _residual(self, x, vq_code):
        """a prepared x minus the centroids of `vq_code`, in a tensor of its own"""
        return (x - self.vq_codec.decode(vq_code)).contiguous()

    def _encode_raw(self, x):
        """(pq_code, vq_code) of a prepared x: the residual's code with pq_use_residual"""
        vq_code = self.vq_codec.encode(x)
        return self.pq_codec.encode(self._residual(x, vq_code) if self.pq_use_residual else x), vq_code

    def encode(self, x):
        """x [d_vector, n] f32 -> packed PQ codes [n_subvectors // 2, n] uint8; with pq_use_residual the pair
        (pq_code, vq_code [n] int64) of the residual x - centroid"""
        x = self._prepare(x)
        return self._encode_raw(x) if self.pq_use_residual else self.pq_codec.encode(x)

    def decode(self, x):
        """packed codes [n_subvectors // 2, n] uint8 -> [d_vector, n] f32; with pq_use_residual `x` is the pair
        (pq_code, vq_code) and the result is centroid + codeword (one fp32 add: what the list scan values)"""
        if self.pq_use_residual:
            assert len(x) == 2
            pq_code, vq_code = x
            assert pq_code.shape[0] * 2 == self.n_subvectors
            assert pq_code.shape[1] == vq_code.shape[0]
            return self.vq_codec.decode(vq_code.to(self.device)) + self.pq_codec.decode(pq_code.to(self.device))
        assert len(x.shape) == 2
        assert x.shape[0] * 2 == self.n_subvectors
        return self.pq_codec.decode(x.to(self.device))

    def add(self, x, ids=None, return_address=False):
        """x [d_vector, n] f32, optional ids [n] int64 (default arange + max_id + 1);
        returns ids (and the slot addresses if return_address)."""
        codes, assigned_cells = self._encode_raw(self._prepare(x))
        return super().add(codes, cells=assigned_cells, ids=ids, return_address=return_address)

    # ---- search ----------------------------------------------------------------------------------------
    def _cell_major_centroids(self):
        """the coarse codebook [d_vector, n_cells] as [n_cells, d_vector] (one centroid per row, what the residual
        scan reads), rebuilt when the codebook changes: the identity-and-version cache of _probe_prepared"""
        cb = self.vq_codec.codebook
        key = (cb.data_ptr(), tuple(cb.shape), util.tensor_version(cb))
        cached = getattr(self, "_centroid_rows_cache", None)
        if cached is None or cached[0] != key or cached[2] is not cb or cb.is_inference():
            self._centroid_rows_cache = cached = (key, cb.t().contiguous(), cb)
        return cached[1]

    def search_cells(self, x, cells, base_sims=None, n_probe_list=None, k=1, return_address=False, _extents=None):
        """Scan the given cells [n_query, n_probe] for each query; (values, ids[, address]).
        (`base_sims` is accepted for IVFPQIndex's signature and unused; `_extents`: the cells' (start, size) when
        the coarse step already gathered them.)"""
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        _extents)
        tables = (self._cell_major_centroids(), cells) if self.pq_use_residual else ()
        vals, address = self._pq4_topk(
            self._storage, x, self.pq_codec.codebook, *tables, cell_start, cell_size, n_probe_list, k,
            is_empty=is_empty, distance=self.distance, slots_hint=slots_hint)
        ids = self.get_id_by_address(address)
        return (vals, ids, address) if return_address else (vals, ids)

    def graphed_search(self, n_query, k=1):
        raise NotImplementedError("GraphedSearch captures IVFPQIndex.search only")

    def search(self, x, k=1, return_address=False):
        """x [d_vector, n_query] f32 -> (values f32 [n_query, k] descending, ids int64 [n_query, k][, address]);
        values are -squared-L2 (euclidean) or the cosine similarity of the PQ reconstruction; (-inf, -1) pads."""
        x = self._prepare(x)
        assert 0 < k <= 1024
        assert self.vq_codec.is_trained and self.pq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        vals, ids, address = self._search_batches(x, lambda xb, sims, cells, n_probe_list, extents: self.search_cells(
            x=xb, cells=cells, base_sims=sims, n_probe_list=n_probe_list, k=k, return_address=True,
            _extents=extents))
        return (vals, ids, address) if return_address else (vals, ids)

    # ---- filtered search ---------------------------------------------------------------------------
    def id_filter(self, ids):
        """ids: an int64 tensor -- one set of allowed ids -- or a sequence of them, one filter row each -> IdFilter,
        what search_filtered takes.  Ids the index does not hold are ignored; the filter follows later add / remove."""
        return IdFilter(self, ids)

    def search_cells_filtered(self, x, cells, flt, filter_of_query=None, base_sims=None, n_probe_list=None, k=1,
                              return_address=False, _extents=None):
        """The k best live codes of the given cells [n_query, n_probe] among the ids `flt` allows; (values, ids[,
        address]).  `filter_of_query`: int32 [n_query], the row of `flt` every query uses (None: row 0).  The table of
        a query (of every probe, with pq_use_residual) is the one search_cells builds.  (`base_sims` is accepted for
        IVFPQIndex's signature and unused; `_extents` as in search_cells.)"""
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        _extents)
        lists = dict(cell_start=cell_start, cell_size=cell_size, n_probe_list=n_probe_list, k=k,
                     filter_bits=flt.bits(self), filter_of_query=filter_of_query, is_empty=is_empty,
                     distance=self.distance, slots_hint=slots_hint)
        if self.pq_use_residual:
            vals, address = self._pq4_filtered.residual(self._storage, x, self.pq_codec.codebook,
                                                        self._cell_major_centroids(), cells, **lists)
        else:
            vals, address = self._pq4_filtered(self._storage, x, self.pq_codec.codebook, **lists)
        ids = self.get_id_by_address(address) if address.numel() else torch.empty_like(address)   # (an empty batch)
        return (vals, ids, address) if return_address else (vals, ids)

    def search_filtered(self, x, k, flt, filter_of_query=None):
        """x [d_vector, n_query] f32, flt = index.id_filter(ids) -> (values f32 [n_query, k] descending, ids int64
        [n_query, k]): the k best stored codes of the query's probed cells (`n_probe`, as in search) AMONG the ids the
        filter allows, padded with (-inf, -1) where fewer exist.  `filter_of_query`: an int tensor [n_query] choosing
        the filter's row per query (a filter made from a sequence of id sets); the default is row 0 for every query.
        A result carries the value search returns for the same code; equal values come by ascending slot address."""
        x = self._prepare(x)
        assert 0 < k <= 1024
        assert self.vq_codec.is_trained and self.pq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        return filtered_search_batches(
            self, x, flt, filter_of_query, lambda xb, rows, sims, cells, n_probe_list, extents:
            self.search_cells_filtered(xb, cells, flt, filter_of_query=rows, base_sims=sims,
                                       n_probe_list=n_probe_list, k=k, _extents=extents))

    # ---- range search ------------------------------------------------------------------------------
    def range_search_cells(self, x, cells, threshold, base_sims=None, n_probe_list=None, return_address=False,
                           _extents=None):
        """Every live code of the given cells [n_query, n_probe] whose value is >= `threshold` (a float, or f32
        [n_query]); (lims, values, ids[, address]) in scan order, see range_search.  The table of a query (of every
        probe, with pq_use_residual) is the one search_cells builds.  (`base_sims` is accepted for IVFPQIndex's
        signature and unused; `_extents` as in search_cells.)"""
        return self._range_cells(x, cells, threshold, n_probe_list, return_address, _extents, None, None)

    def range_search_cells_filtered(self, x, cells, threshold, flt, filter_of_query=None, base_sims=None,
                                    n_probe_list=None, return_address=False, _extents=None):
        """range_search_cells among the ids `flt` allows; `filter_of_query`: int32 [n_query], the row of `flt` every
        query uses (None: row 0), as in search_cells_filtered.  The bit rows carry a row per query: one pair of passes
        whatever rows the queries name."""
        assert isinstance(flt, IdFilter), "flt is what index.id_filter(ids) returns"
        return self._range_cells(x, cells, threshold, n_probe_list, return_address, _extents, flt, filter_of_query)

    def _range_cells(self, x, cells, threshold, n_probe_list, return_address, extents, flt, filter_of_query):
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        extents)
        lists = dict(cell_start=cell_start, cell_size=cell_size, n_probe_list=n_probe_list, threshold=threshold,
                     filter_bits=None if flt is None else flt.bits(self), filter_of_query=filter_of_query,
                     is_empty=is_empty, distance=self.distance)
        if self.pq_use_residual:
            lims, vals, address = self._pq4_range.residual(self._storage, x, self.pq_codec.codebook,
                                                           self._cell_major_centroids(), cells, **lists)
        else:
            lims, vals, address = self._pq4_range(self._storage, x, self.pq_codec.codebook, slots_hint=slots_hint,
                                                  **lists)
        ids = self.get_id_by_address(address) if address.numel() else torch.empty_like(address)
        return (lims, vals, ids, address) if return_address else (lims, vals, ids)

    def range_search(self, x, threshold, return_address=False, sort=False):
        """x [d_vector, n_query] f32, threshold a float or f32 [n_query] -> (lims int64 [n_query + 1], values f32
        [total], ids int64 [total][, address]): the hits of query q are values[lims[q]:lims[q+1]] and
        ids[lims[q]:lims[q+1]] -- every stored code of the query's probed cells (`n_probe`, as in search) whose value is
        >= threshold.  `threshold` is in the index's value space, the one search returns: -squared-L2 to the PQ
        reconstruction for "euclidean" (everything within distance r: threshold = -r * r), the cosine similarity of
        the reconstruction for "cosine".  A hit carries the bits search returns for the same slot.
        Hits come in scan order (probe rank, then slot address); sort=True orders each query's hits by value
        descending, equal values by address ascending.  Synchronises once per batch of `max_query_batch` queries:
        the number of hits sizes the outputs."""
        x = self._prepare(x)
        assert self.vq_codec.is_trained and self.pq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        return range_search_batches(
            self, x, threshold, lambda xb, thr, sims, cells, n_probe_list, extents: self.range_search_cells(
                xb, cells, thr, base_sims=sims, n_probe_list=n_probe_list, return_address=True, _extents=extents),
            return_address, sort)

    def range_search_filtered(self, x, threshold, flt, filter_of_query=None, return_address=False, sort=False):
        """range_search among the ids a filter allows: flt = index.id_filter(ids), `filter_of_query` (an int tensor
        [n_query]) chooses its row per query as in search_filtered (default: row 0; a row outside [0, n_filters) has
        no hit).  The same values, order and outputs as range_search.  One pair of passes, and one synchronisation,
        per batch of `max_query_batch` queries, whatever rows its queries name."""
        x = self._prepare(x)
        assert self.vq_codec.is_trained and self.pq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        rows = checked_filter_rows(self, x, flt, filter_of_query)
        return range_search_batches(
            self, x, threshold, lambda xb, thr, rows_b, sims, cells, n_probe_list, extents:
            self.range_search_cells_filtered(xb, cells, thr, flt, rows_b, base_sims=sims, n_probe_list=n_probe_list,
                                             return_address=True, _extents=extents),
            return_address, sort, alongside=(rows,))
