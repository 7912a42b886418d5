"""IVFPQIndex: drop-in for torchpq.index.IVFPQIndex (reference index/IVFPQIndex.py:12-524).

Same constructor, methods, properties, asserts, tensor layouts ([d_vector, n] fp32 in, ids
int64 out, values descending with (-inf, -1) padding) and state_dict keys.  Everything below
the Python API runs in hand-written HIP kernels for gfx950 (libtorchpq_amd.so); the only
library math is the coarse query x cell-centroid GEMM and the one-off residual tables
(rocBLAS via torch.matmul/bmm, as the reference uses cuBLAS).
"""
import torch

from .. import util
from ..codec import PQCodec
from ..container import CellContainer
from ..fn import IVFPQTopk
from ..kernels import PACKED_M, CellKeptState, IVFPQFilteredTopkHip, IVFPQRangeHip, ResidualPart1Hip, ResidualSlotTermsHip
from ._coarse import CoarseProbeMixin
from ._filter import IdFilter, filtered_search_batches
from ._range import range_search_batches


class IVFPQIndex(CoarseProbeMixin, CellContainer):
    # search keeps the scan-layout copy of the codes at every m that has a kernel instantiation:
    # long codes gain from bank-conflict-free look-ups (m >= 56: 1.2-1.7x), short and medium ones
    # from several slots per lane per iteration (r02 sweep, scan layout vs reference layout:
    # m=28 1.97 vs 2.25 ms, 32 1.98 vs 2.19, 40 2.37 vs 2.67, 48 2.65 vs 2.94 per 10 000 queries).
    # (m with packed_max_short_subvectors < m < packed_min_subvectors would use the reference layout)
    packed_min_subvectors = 0
    packed_max_short_subvectors = 24
    # the LUT is built inside the scan workgroups (no [m, nq, 256] table in HBM) up to this
    # sub-vector length; the workgroup then reads m * ds KiB of L2-resident codebook per query
    fused_lut_max_subvector = 4
    use_cell_major = True
    use_cell_threshold = True
    use_cell_single_product = True
    use_cell_kept = True

    def __init__(self, d_vector, n_subvectors=8, n_cells=128, initial_size=None,
                 expand_step_size=128, expand_mode="double", distance="euclidean",
                 device="cuda:0", pq_use_residual=False, verbose=0):
        if torch.device(device).type == "cuda":
            assert torch.cuda.is_available(), "cuda is not available"
            assert n_subvectors <= util.max_subvectors()
        assert d_vector % n_subvectors == 0
        assert n_subvectors % 4 == 0, "codes are stored 4 sub-quantizers per word (contiguous_size=4)"
        assert distance in ("euclidean", "cosine"), \
            "euclidean and cosine work end to end (MultiKMeans.py:82-113)"
        super().__init__(code_size=n_subvectors, n_cells=n_cells, dtype="uint8", device=device,
                         initial_size=initial_size, expand_step_size=expand_step_size,
                         expand_mode=expand_mode, use_inverse_id_mapping=True, contiguous_size=4,
                         verbose=verbose)
        self.d_vector = d_vector
        self.n_subvectors = n_subvectors
        self.d_subvector = d_vector // n_subvectors
        self.distance = distance
        self.verbose = verbose
        self.pq_use_residual = pq_use_residual
        # residual search keeps a [n_cells, m, 256] table when it fits 4 GiB (IVFPQIndex.py:52-55)
        self._use_precomputed = bool(pq_use_residual and
                                     (n_cells * 256 * n_subvectors * 4) <= 4 * 1024 ** 3)
        self._precomputed_part2 = None
        self._part2_by_cell = None       # [n_cells, m, 256] contiguous copy for the scan kernels
        self._slot_terms = None          # (codes version, slot_term [capacity], cell_bound [n_cells])
        self._use_cublas = True
        self._use_tensor_core = False
        self._fp16_scale_mode = "a"
        self.use_packed_layout = True   # MI355X scan layout (bank-conflict-free LDS look-ups)
        self.use_fused_lut = True       # build the ADC LUT inside the scan workgroups (no HBM table)
        # hand the probed cells to the fused scan: a large cell-dense batch at m = 64 may then take the cell-major
        # form (csrc/scan_cells.hip; the library's rule decides, IVFPQTopkHip.last_cell_major() tells)
        self.use_cell_major = True
        # ... and that form may take its threshold from the candidate kernel's group maxima instead of a query-major pass
        # over the first probes (the library's rule decides, IVFPQTopkHip.last_cell_threshold() tells)
        self.use_cell_threshold = True
        # ... whose selection key is one fp16 product per k-step with a per-query band (ds = 2); False: three products and
        # the narrower band -- same results; for data with many rows within that band of the k-th best, whose queries
        # would overflow their lists and be redone exactly (IVFPQTopkHip.last_cell_products() tells)
        self.use_cell_single_product = True
        # ... and keeps what it derives from codes, codebook and tombstones alone -- scale, split codebook, slot norms --
        # across searches, rebuilt after add / remove / growth / load_state_dict / a write to the codebook
        # (IVFPQTopkHip.last_cell_kept tells; False: derived again in every call)
        self.use_cell_kept = True
        self._cell_kept = None           # kernels.CellKeptState, keyed on what it was derived from
        self._cell_kept_built = 0        # builds of the states dropped so far

        self._init_coarse(n_cells, verbose)
        self.pq_codec = PQCodec(d_vector=d_vector, n_subvectors=n_subvectors, n_clusters=256,
                                distance=distance, verbose=verbose)
        self._ivfpq_topk = IVFPQTopk(n_subvectors=n_subvectors, contiguous_size=self.contiguous_size)
        self._ivfpq_range = IVFPQRangeHip(m=n_subvectors)
        self._ivfpq_filtered = IVFPQFilteredTopkHip(m=n_subvectors)
        self.to(device)

    # ---- knobs (reference :89-232) ---------------------------------------------------------------
    @property
    def use_cublas(self):
        return self._use_cublas

    @use_cublas.setter
    def use_cublas(self, value):
        assert type(value) is bool
        self._use_cublas = value

    @property
    def use_tensor_core(self):
        return self._use_tensor_core

    @use_tensor_core.setter
    def use_tensor_core(self, value):
        """True: the coarse step SELECTS on the fp16 matrix cores wherever the shape allows it (d <= 128) and
        gives every candidate cell the fp32 kernel's own similarity -- the cells, their order and the
        similarities are unchanged, bit for bit (the reference's knob, :98-125, trades accuracy for the speed).
        False (default): the library's thresholds decide (the same pass from 2 048 cells on)."""
        assert type(value) is bool
        assert self.use_cublas
        self._use_tensor_core = value
        self._coarse_probe.route = "fp16" if value else "auto"

    @property
    def fp16_scale_mode(self):
        return self._fp16_scale_mode

    @fp16_scale_mode.setter
    def fp16_scale_mode(self, value):
        assert value in ["a", "b", "both", "none"]
        self._fp16_scale_mode = value

    @property
    def use_precomputed(self):
        return self._use_precomputed

    @use_precomputed.setter
    def use_precomputed(self, value):
        assert type(value) is bool
        if value:
            assert self.pq_use_residual, " `use_precomputed=True` is only valid when `pq_use_residual` is True"
            assert (self.pq_codec.is_trained and self.vq_codec.is_trained), "index is not trained"
            self.precompute_part2()
        else:
            self._drop_part2()
        self._use_precomputed = value

    def _drop_part2(self):
        self._precomputed_part2 = None
        self._part2_by_cell = None
        self._slot_terms = None

    def precompute_part2(self):
        """[m, n_cells, 256]: -2 c_j . r_jc - |r_jc|^2 (reference :160-170; one-off library bmm)"""
        pq_codebook = self.pq_codec.codebook
        vq_codebook = self.vq_codec.codebook.reshape(self.n_subvectors, self.d_subvector, self.n_cells)
        part2 = (torch.bmm(vq_codebook.transpose(-1, -2), pq_codebook) * -2
                 - pq_codebook.norm(dim=1).pow(2)[:, None])
        # one resident copy, in the [n_cells, m, 256] order the scan kernels read;
        # `_precomputed_part2` keeps the reference's [m, n_cells, 256] shape as a view of it
        self._part2_by_cell = part2.transpose(0, 1).contiguous()
        del part2
        self._precomputed_part2 = self._part2_by_cell.transpose(0, 1)
        self._slot_terms = None

    def _residual_slot_terms(self):
        """(slot_term, cell_bound) of the packed residual scan, rebuilt when the codes changed"""
        if self._slot_terms is None or self._slot_terms[0] != self._codes_version:
            st, cb = ResidualSlotTermsHip()(self._storage, self._part2_by_cell, self._cell_start,
                                            self._cell_size)
            self._slot_terms = (self._codes_version, st, cb)
        return self._slot_terms[1], self._slot_terms[2]

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

    def _cell_kept_state(self, n_bytes, device):
        """the kept state of the cell-major form for the index as it stands: the one in hand while codes, codebook and
        tombstones are what it was derived from (version counters and the buffers' identity), else a new, not yet valid
        one, which the calling search builds.  None inside a stream capture that finds no valid state."""
        def ident(t):
            return None if t is None else (t.data_ptr(), tuple(t.shape), util.tensor_version(t), str(t.device))
        key = (self._codes_version, bool(self._has_holes), ident(self.pq_codec.codebook), ident(self._storage),
               ident(self._is_empty))
        st = self._cell_kept
        if st is not None and st.key == key and st.buf.numel() >= n_bytes and st.buf.device == torch.device(device):
            return st
        if torch.cuda.is_current_stream_capturing():
            return None
        self._drop_cell_kept()
        self._cell_kept = CellKeptState(n_bytes, device, key)
        return self._cell_kept

    def _drop_cell_kept(self):
        if self._cell_kept is not None:
            self._cell_kept_built += self._cell_kept.builds
        self._cell_kept = None

    @property
    def cell_kept_builds(self):
        """diagnostics: how often a search built the kept state so far"""
        return self._cell_kept_built + (0 if self._cell_kept is None else self._cell_kept.builds)

    def to(self, *args, **kwargs):
        if getattr(self, "_cell_kept", None) is not None:   # (a state describes buffers of the device it is on)
            self._drop_cell_kept()
        return super().to(*args, **kwargs)

    def _after_load_state_dict(self):
        self.to(self.device)
        self._drop_part2()
        self._drop_cell_kept()
        super()._after_load_state_dict()

    # ---- train / encode / add (reference :234-364) ------------------------------------------------
    def train(self, x, force_retrain=False):
        """x [d_vector, n_data] f32: coarse k-means (n_cells) then 256-centroid PQ codebooks."""
        if self.vq_codec.is_trained and self.pq_codec.is_trained and not force_retrain:
            self.print_message("index is already trained", 1)
            return
        x = self._prepare(x)
        self.print_message("start training VQ codec...", 1)
        code = self.vq_codec.train(x)
        self.print_message("start training PQ codec...", 1)
        if self.pq_use_residual:
            # PQ is learnt on x - centroid(x); the caller's tensor is left untouched (the reference
            # subtracts and re-adds in place, :246-254)
            self.pq_codec.train((x - self.vq_codec.decode(code)).contiguous())
            self._drop_part2()
        else:
            self.pq_codec.train(x)
        self.print_message("index is trained successfully!", 1)

    def encode(self, x):
        """x [d_vector, n] f32 -> PQ codes [n_subvectors, n] uint8"""
        x = self._prepare(x)
        if self.pq_use_residual:  # (pq_code, vq_code) of the residual x - centroid (:276-281)
            return self._encode_raw(x)
        return self.pq_codec.encode(x)

    def decode(self, x):
        """codes [n_subvectors, n] uint8 -> [d_vector, n] f32; with pq_use_residual `x` is the
        pair (pq_code, vq_code) and the result is centroid + decoded residual (:301-309)"""
        if self.pq_use_residual:
            assert len(x) == 2
            pq_code, vq_code = x
            assert pq_code.shape[0] == self.n_subvectors
            assert pq_code.shape[1] == vq_code.shape[0]
            return self.vq_codec.decode(vq_code.to(self.device)) + self.pq_codec.decode(pq_code.to(self.device))
        assert len(x.shape) == 2
        assert x.shape[0] == self.n_subvectors
        return self.pq_codec.decode(x.to(self.device))

    def add(self, x, ids=None, return_address=False):
        """x [d_vector, n] f32, optional ids [n] int64 (default arange + max_id + 1);
        returns ids (and the slot addresses if return_address)."""
        x = self._prepare(x)
        if self.pq_use_residual:
            codes, assigned_cells = self._encode_raw(x)
        else:
            assigned_cells = self.vq_codec.encode(x)
            codes = self.pq_codec.encode(x)
        return super().add(codes, cells=assigned_cells, ids=ids, return_address=return_address)

    def _encode_raw(self, x):
        """residual encode of an already normalised x"""
        vq_code = self.vq_codec.encode(x)
        return self.pq_codec.encode((x - self.vq_codec.decode(vq_code)).contiguous()), vq_code

    # ---- residual tables (reference :366-405) -----------------------------------------------------
    def precomputed_adc_residual_precomputed(self, x):
        """(part1 [n_query, m, 256] = 2 q_j.r_jc,  part2 [n_cells, m, 256])"""
        part1 = ResidualPart1Hip()(x, self.pq_codec.codebook)
        if self._precomputed_part2 is None:
            self.precompute_part2()
        return part1, self._part2_by_cell

    def precomputed_adc_residual(self, x, cells):
        """[n_query, n_probe, m, 256]: one LUT per (query, probe); memory-hungry, used only when
        the part2 table is disabled (use_precomputed=False)"""
        n_query, n_probe = cells.shape
        pq_codebook = self.pq_codec.codebook
        xs = x.reshape(self.n_subvectors, self.d_subvector, n_query).transpose(-1, -2)
        part1 = 2 * (xs @ pq_codebook).permute(1, 0, 2) - pq_codebook.norm(dim=1).pow(2)[None]
        vq = self.vq_codec.codebook.reshape(self.n_subvectors, self.d_subvector, self.n_cells)
        vq = vq[:, :, cells].permute(0, 2, 3, 1)                       # [m, nq, n_probe, ds]
        part2 = -2 * (vq @ pq_codebook[:, None].expand(-1, n_query, -1, -1))  # [m, nq, n_probe, 256]
        return (part1[:, None] + part2.permute(1, 2, 0, 3)).contiguous()

    # ---- search (reference :407-524) ---------------------------------------------------------------
    def _scan_layout(self):
        """the scan-layout copy of the codes for the plain scan, or None where the reference layout is kept (the
        class attributes above)"""
        m = self.n_subvectors
        if self.use_packed_layout and m in PACKED_M and (
                m >= self.packed_min_subvectors or m <= self.packed_max_short_subvectors):
            return self.packed_storage()
        return None

    def search_cells(self, x, cells, base_sims=None, n_probe_list=None, k=1, return_address=False,
                     _extents=None):
        """Scan the given cells [n_query, n_probe] for each query; (values, ids[, address]).
        (`_extents`: the cells' (start, size) when the coarse step already gathered them.)"""
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        _extents)
        lists = dict(data=self._scan_codes(), cell_start=cell_start, cell_size=cell_size, is_empty=is_empty,
                     n_probe_list=n_probe_list, address2id=self._address2id)
        # the fused paths re-read the codebook (m*ds KiB, L2-resident) per workgroup instead of a
        # 1-KiB-per-sub-quantizer LUT row from HBM: a win while the sub-vectors are short
        fused = self.use_fused_lut and self.d_subvector <= self.fused_lut_max_subvector
        if self.pq_use_residual:
            assert base_sims is not None, "base_sims is required when pq_use_residual is True"
            if self.use_precomputed and self.use_packed_layout and self.n_subvectors in PACKED_M:
                # scan layout: part1[q] staged once per query (built in the workgroup while the
                # sub-vectors are short), the cell-dependent half folded into a per-slot constant
                if self._precomputed_part2 is None:
                    self.precompute_part2()
                slot_term, cell_bound = self._residual_slot_terms()
                part1 = None if fused else self.precomputed_adc_residual_precomputed(x)[0]
                found = self._ivfpq_topk._scan.topk_residual_packed(
                    packed=self.packed_storage(), part2=self._part2_by_cell, slot_term=slot_term,
                    cell_bound=cell_bound, cells=cells, base_sims=base_sims, n_candidates=k, part1=part1,
                    query=x if fused else None, codebook=self.pq_codec.codebook if fused else None,
                    slots_hint=slots_hint, **lists)
            elif self.use_precomputed:
                part1, part2 = self.precomputed_adc_residual_precomputed(x)
                found = self._ivfpq_topk.topk_residual_precomputed(
                    part1=part1, part2=part2, cells=cells, base_sims=base_sims, k=k, **lists)
            else:
                found = self._ivfpq_topk.topk_residual(
                    base_sims=base_sims, precomputed=self.precomputed_adc_residual(x, cells), k=k, **lists)
        elif fused:
            found = self._ivfpq_topk.topk_fused(
                packed=self._scan_layout(), query=x, codebook=self.pq_codec.codebook, k=k, distance=self.distance,
                slots_hint=slots_hint, cells=cells if self.use_cell_major else None, n_cells=self.n_cells,
                cell_threshold=self.use_cell_threshold, cell_single_product=self.use_cell_single_product,
                kept=self._cell_kept_state if self.use_cell_kept and self.use_cell_major else None, **lists)
        else:
            found = self._ivfpq_topk.topk(
                packed=self._scan_layout(), precomputed=self.pq_codec.precompute_adc(x), k=k,
                slots_hint=slots_hint, **lists)
        topk_val, topk_address, topk_ids = found
        return (topk_val, topk_ids, topk_address) if return_address else (topk_val, topk_ids)

    def graphed_search(self, n_query, k=1):
        """search() for a fixed batch shape captured in one HIP graph (low-latency serving)"""
        from .graphed import GraphedSearch
        return GraphedSearch(self, n_query, k)

    def search(self, x, k=1, return_address=False):
        """x [d_vector, n_query] f32 -> (values f32 [n_query, k] descending, ids int64 [n_query, k]);
        values are -squared-L2 (euclidean) or cosine similarity of the PQ reconstruction.
        `return_address` is accepted and ignored, as in the reference (:521)."""
        x = self._prepare(x)
        assert 0 < k <= 1024
        assert self.vq_codec.is_trained and self.pq_codec.is_trained, "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells
        return self._search_batches(x, lambda xb, sims, cells, n_probe_list, extents: self.search_cells(
            x=xb, cells=cells, base_sims=sims, n_probe_list=n_probe_list, k=k, return_address=False,
            _extents=extents))

    # ---- range search ------------------------------------------------------------------------------
    def range_search_cells(self, x, cells, threshold, base_sims=None, n_probe_list=None, return_address=False,
                           _extents=None):
        """Every live code of the given cells [n_query, n_probe] whose value is >= `threshold` (a float, or f32
        [n_query]); (lims, values, ids[, address]) in scan order, see range_search.  The tables are those search_cells
        would use; the codes are read in the container's own layout (`_scan_codes()`), never the scan-layout copy.
        (`_extents` as in search_cells.)"""
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        _extents)
        lists = dict(data=self._scan_codes(), cell_start=cell_start.contiguous(), cell_size=cell_size.contiguous(),
                     n_probe_list=n_probe_list, threshold=threshold, is_empty=is_empty)
        fused = self.use_fused_lut and self.d_subvector <= self.fused_lut_max_subvector
        if self.pq_use_residual:
            assert base_sims is not None, "base_sims is required when pq_use_residual is True"
            if self.use_precomputed:
                if self._precomputed_part2 is None:
                    self.precompute_part2()
                tables = dict(part2=self._part2_by_cell, cells=cells)
                if fused:
                    tables.update(query=x, codebook=self.pq_codec.codebook)
                else:
                    tables.update(part1=ResidualPart1Hip()(x, self.pq_codec.codebook))
            else:
                tables = dict(full=self.precomputed_adc_residual(x, cells))
            lims, vals, address = self._ivfpq_range.residual(base_sims=base_sims, **tables, **lists)
        elif fused:
            lims, vals, address = self._ivfpq_range(query=x, codebook=self.pq_codec.codebook, distance=self.distance,
                                                    slots_hint=slots_hint, **lists)
        else:
            lims, vals, address = self._ivfpq_range(precomputed=self.pq_codec.precompute_adc(x),
                                                    slots_hint=slots_hint, **lists)
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

    # ---- filtered search ---------------------------------------------------------------------------
    def id_filter(self, ids):
        """ids: an int64 tensor -- one set of allowed ids -- or a sequence of them, one filter row each -> IdFilter,
        what search_filtered takes.  Ids the index does not hold are ignored; the filter follows later add / remove."""
        return IdFilter(self, ids)

    def search_cells_filtered(self, x, cells, flt, filter_of_query=None, base_sims=None, n_probe_list=None, k=1,
                              return_address=False, _extents=None):
        """The k best live codes of the given cells [n_query, n_probe] among the ids `flt` allows; (values, ids[,
        address]).  `filter_of_query`: int32 [n_query], the row of `flt` every query uses (None: row 0).  The tables
        are those search_cells would use; the codes are read in the container's own layout (`_scan_codes()`), never
        the scan-layout copy.  (`_extents` as in search_cells.)"""
        n_probe_list, cell_start, cell_size, slots_hint, is_empty = self._scan_preamble(x, cells, n_probe_list,
                                                                                        _extents)
        lists = dict(data=self._scan_codes(), cell_start=cell_start, cell_size=cell_size, n_probe_list=n_probe_list,
                     k=k, filter_bits=flt.bits(self), filter_of_query=filter_of_query, is_empty=is_empty,
                     address2id=self._address2id)
        fused = self.use_fused_lut and self.d_subvector <= self.fused_lut_max_subvector
        if self.pq_use_residual:
            assert base_sims is not None, "base_sims is required when pq_use_residual is True"
            if self.use_precomputed:
                if self._precomputed_part2 is None:
                    self.precompute_part2()
                tables = dict(part2=self._part2_by_cell, cells=cells)
                if fused:
                    tables.update(query=x, codebook=self.pq_codec.codebook)
                else:
                    tables.update(part1=ResidualPart1Hip()(x, self.pq_codec.codebook))
            else:
                tables = dict(full=self.precomputed_adc_residual(x, cells))
            vals, address, ids = self._ivfpq_filtered.residual(base_sims=base_sims, **tables, **lists)
        elif fused:
            vals, address, ids = self._ivfpq_filtered(query=x, codebook=self.pq_codec.codebook,
                                                      distance=self.distance, slots_hint=slots_hint, **lists)
        else:
            vals, address, ids = self._ivfpq_filtered(precomputed=self.pq_codec.precompute_adc(x),
                                                      slots_hint=slots_hint, **lists)
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
