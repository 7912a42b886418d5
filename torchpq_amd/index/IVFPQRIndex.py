"""IVFPQRIndex: IVFPQ with a second, re-rank product quantizer (Jegou et al., "Searching in one billion
vectors: re-rank with source coding").

Constructor, storage layout, sub-modules and state_dict keys follow the reference's new-API class
(torchpq/index/IVFPQRIndex.py:7-222), whose `search` is unfinished (:229 raises); train / encode / decode /
search semantics follow the finished legacy class (torchpq/legacy/IVFPQR.py:278-482).

The first stage is IVFPQIndex's search path on the leading `n_subvectors` code rows of the container, asked
for `k * rerank_factor` slot addresses; the second stage (tpq_ivfpqr_rerank, csrc/rerank.hip) re-values those
candidates from both codes of their slot and keeps the best k.
"""
import torch

from .. import util
from ..codec import PQCodec
from ..kernels import IVFPQRerankHip
from .IVFPQIndex import IVFPQIndex


class IVFPQRIndex(IVFPQIndex):
    def __init__(self, d_vector, n_subvectors=8, n_subvectors_rerank=8, n_cells=128, use_residual=True,
                 initial_size=None, expand_step_size=128, expand_mode="double", distance="euclidean",
                 device="cuda:0", verbose=0, rerank_factor=2):
        assert n_subvectors_rerank % 4 == 0, "codes are stored 4 sub-quantizers per word (contiguous_size=4)"
        assert d_vector % n_subvectors_rerank == 0
        if torch.device(device).type == "cuda":
            assert torch.cuda.is_available(), "cuda is not available"
            assert n_subvectors_rerank <= util.max_subvectors()
        # the first stage is an IVFPQIndex whose PQ is not residual to the coarse centroid (the reference class
        # has no pq_use_residual); its container is then widened by the re-rank rows
        super().__init__(d_vector, n_subvectors=n_subvectors, n_cells=n_cells, initial_size=initial_size,
                         expand_step_size=expand_step_size, expand_mode=expand_mode, distance=distance,
                         device=device, pq_use_residual=False, verbose=verbose)
        self.n_subvectors_rerank = n_subvectors_rerank
        self.use_residual = use_residual
        self.rerank_factor = rerank_factor
        self.code_size = n_subvectors + n_subvectors_rerank
        self._storage = torch.zeros(self.code_size // self.contiguous_size, self.capacity, self.contiguous_size,
                                    device=self._storage.device, dtype=self.dtype)
        self.pq_rerank_codec = PQCodec(d_vector=d_vector, n_subvectors=n_subvectors_rerank, n_clusters=256,
                                       distance=distance, verbose=verbose)
        self._rerank = IVFPQRerankHip()
        self.to(device)

    # ---- knobs (reference :74-99) ------------------------------------------------------------------
    @property
    def rerank_factor(self):
        return self._rerank_factor

    @rerank_factor.setter
    def rerank_factor(self, value):
        """the list scan returns k * rerank_factor candidates (legacy/IVFPQR.py:20); 1 = re-order the k"""
        assert type(value) is int and value >= 1
        self._rerank_factor = value

    def _codec_setter(codec, attr):
        def setter(self, value):
            setattr(getattr(self, codec).kmeans, attr, value)
        return setter

    set_vq_codec_max_iter = _codec_setter("vq_codec", "max_iter")
    set_vq_codec_n_redo = _codec_setter("vq_codec", "n_redo")
    set_vq_codec_tolerance = _codec_setter("vq_codec", "tol")
    set_pq_codec_max_iter = _codec_setter("pq_codec", "max_iter")
    set_pq_codec_n_redo = _codec_setter("pq_codec", "n_redo")
    set_pq_codec_tolerance = _codec_setter("pq_codec", "tol")
    set_pq_rerank_codec_max_iter = _codec_setter("pq_rerank_codec", "max_iter")
    set_pq_rerank_codec_n_redo = _codec_setter("pq_rerank_codec", "n_redo")
    set_pq_rerank_codec_tolerance = _codec_setter("pq_rerank_codec", "tol")
    del _codec_setter

    # ---- the scan reads the first-stage rows only ----------------------------------------------------
    def _scan_codes(self):
        """[n_subvectors / 4, capacity, 4]: a contiguous leading view of the container's rows (the scan-layout
        copy then holds the FIRST-STAGE rows only)"""
        return self._storage[:self.n_subvectors // self.contiguous_size]

    def set_data_by_address(self, data, address):
        # the container's scatter would update the scan-layout copy as if it held all code_size rows:
        # mark it stale instead, the next search repacks the leading rows
        self._packed_valid = False
        super().set_data_by_address(data, address)

    # ---- train / encode / decode / add (reference :101-222, legacy/IVFPQR.py:278-350) ----------------
    def train(self, x, force_retrain=False):
        """x [d_vector, n_data] f32: coarse k-means, the first-stage PQ on x, then the re-rank PQ on the
        first stage's quantisation residual x - pq_codec.decode(code) (on x itself if not use_residual), as
        legacy/IVFPQR.py:298-313.  (Line 124 of the reference's new-API file trains `pq_codec` a second time
        and never `pq_rerank_codec`: a slip, not reproduced.)"""
        if (self.vq_codec.is_trained and self.pq_codec.is_trained and self.pq_rerank_codec.is_trained
                and not force_retrain):
            self.print_message("index is already trained", 1)
            return
        x = self._prepare(x)
        self.print_message("start training VQ codec...", 1)
        self.vq_codec.train(x)
        self.print_message("start training PQ codec...", 1)
        code = self.pq_codec.train(x)
        if self.use_residual:
            self.print_message("start training PQ Rerank codec with residuals...", 1)
            self.pq_rerank_codec.train((x - self.pq_codec.decode(code.byte())).contiguous())
        else:
            self.print_message("start training PQ Rerank codec...", 1)
            self.pq_rerank_codec.train(x)
        self.print_message("index is trained successfully!", 1)

    def _encode_normalised(self, x):
        y1 = self.pq_codec.encode(x)
        if self.use_residual:
            x = (x - self.pq_codec.decode(y1)).contiguous()
        return torch.cat([y1, self.pq_rerank_codec.encode(x)], dim=0)

    def encode(self, x):
        """x [d_vector, n] f32 -> codes [n_subvectors + n_subvectors_rerank, n] uint8"""
        return self._encode_normalised(self._prepare(x))

    def decode(self, x):
        """codes [n_subvectors + n_subvectors_rerank, n] uint8 -> [d_vector, n] f32"""
        assert len(x.shape) == 2
        assert x.shape[0] == self.n_subvectors + self.n_subvectors_rerank
        x = x.to(self.device)
        y = self.pq_rerank_codec.decode(x[self.n_subvectors:])
        if self.use_residual:
            y = y + self.pq_codec.decode(x[:self.n_subvectors])
        return y

    def add(self, x, ids=None, return_address=False):
        """x [d_vector, n] f32, optional ids [n] int64 (default arange + max_id + 1);
        returns ids (and the slot addresses if return_address)."""
        x = self._prepare(x)
        assigned_cells = self.vq_codec.encode(x)
        # (the reference's `super(IVFPQIndex, self).add`, :217, names a class its file never imports)
        return super(IVFPQIndex, self).add(self._encode_normalised(x), cells=assigned_cells, ids=ids,
                                           return_address=return_address)

    # ---- search ----------------------------------------------------------------------------------------
    def graphed_search(self, n_query, k=1):
        raise NotImplementedError("GraphedSearch captures IVFPQIndex.search only")

    def search(self, x, k=1, return_address=False):
        """x [d_vector, n_query] f32 -> (values f32 [n_query, k] descending, ids int64 [n_query, k]
        [, address int64 [n_query, k]]).  The list scan of IVFPQIndex returns k * rerank_factor candidates by
        the first code; they are re-ranked by -|q - (decode(c) + decode_r(c_r))|^2 (the dot product for
        "cosine"), or by the ADC value of the re-rank code alone when not use_residual."""
        x = self._prepare(x)
        assert 0 < k <= 1024
        k1 = k * self.rerank_factor
        assert k1 <= 1024, f"k * rerank_factor = {k1} exceeds the list scan's limit of 1024 candidates"
        assert (self.vq_codec.is_trained and self.pq_codec.is_trained
                and self.pq_rerank_codec.is_trained), "index is not trained"
        assert 1 <= self.n_probe <= self.n_cells

        def per_batch(xb, sims, cells, n_probe_list, extents):
            _, _, candidates = self.search_cells(x=xb, cells=cells, base_sims=sims, n_probe_list=n_probe_list, k=k1,
                                                 return_address=True, _extents=extents)
            v, a, i = self._rerank(self._storage, self.n_subvectors, self.pq_codec.codebook,
                                   self.pq_rerank_codec.codebook, xb, candidates, k,
                                   use_residual=self.use_residual, distance=self.distance,
                                   address2id=self._address2id)
            return v, i, a

        vals, ids, address = self._search_batches(x, per_batch)
        return (vals, ids, address) if return_address else (vals, ids)

    # ---- range search ----------------------------------------------------------------------------------
    def range_search_cells(self, x, cells, threshold, base_sims=None, n_probe_list=None, return_address=False,
                           _extents=None):
        raise NotImplementedError(
            "IVFPQRIndex has no range search: the list scan's values are those of the first code, not the re-ranked "
            "values search returns, so a threshold in this index's value space cannot be applied to them")

    def range_search(self, x, threshold, return_address=False, sort=False):
        raise NotImplementedError(
            "IVFPQRIndex has no range search: the list scan's values are those of the first code, not the re-ranked "
            "values search returns, so a threshold in this index's value space cannot be applied to them")

    # ---- filtered search -------------------------------------------------------------------------------
    def search_cells_filtered(self, x, cells, flt, filter_of_query=None, base_sims=None, n_probe_list=None, k=1,
                              return_address=False, _extents=None):
        raise NotImplementedError(
            "IVFPQRIndex has no filtered search: the filtered list scan returns the values of the first code, not the "
            "re-ranked values search returns")

    def search_filtered(self, x, k, flt, filter_of_query=None):
        raise NotImplementedError(
            "IVFPQRIndex has no filtered search: the filtered list scan returns the values of the first code, not the "
            "re-ranked values search returns")
