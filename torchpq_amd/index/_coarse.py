"""The coarse step of the IVF indexes (IVFPQIndex and its subclasses, IVFFlatIndex): the probed cells of a query batch.

The host class is a CellContainer with `d_vector`, `distance` and the switch `use_cublas`; `_init_coarse` sets up the
rest.  Besides the coarse step, the halves of `add` / `search` / `search_cells` that the IVF indexes share live here:
the preparation of a [d_vector, n] input, the preamble of a list scan, the loop over query batches.
"""
import torch

from .. import metric, util
from ..codec import VQCodec
from ..fn import Topk
from ..kernels import CoarseProbeHip, CoarseSelectHip, SmartProbingHip


class CoarseProbeMixin:
    def _init_coarse(self, n_cells, verbose):
        """the coarse-step members; called where the index registers its sub-modules (`vq_codec` comes first in
        every state_dict())"""
        self.n_probe = 1
        self._use_smart_probing = True
        self._smart_probing_temperature = 30.0
        self.use_fused_probe = True     # coarse sims + select + list extents + probe count: one call
        # bounds what a batch allocates: the coarse step's [n_query, n_cells] matrix, IVFPQIndex's [m, nq, 256] LUT
        # (m=64: 2 GiB per batch)
        self.max_query_batch = 32768
        self.vq_codec = VQCodec(n_clusters=n_cells, n_redo=1, max_iter=15, tol=1e-4,
                                distance="euclidean", init_mode="random", verbose=verbose)
        self._topk = Topk()
        self._smart_probing = SmartProbingHip()
        self._coarse_select = CoarseSelectHip()
        self._coarse_probe = CoarseProbeHip()

    def _prepare(self, x):
        """a [d_vector, n] input as the kernels take it: on the index's device, normalised for "cosine", contiguous"""
        assert len(x.shape) == 2
        assert x.shape[0] == self.d_vector
        x = x.to(self.device)
        if self.distance == "cosine":
            x = util.normalize(x)
        return x.contiguous()

    def _scan_preamble(self, x, cells, n_probe_list, extents):
        """what every search_cells hands its list scan: (n_probe_list, cell_start, cell_size, slots_hint, is_empty);
        `extents`: the cells' (start, size) when the coarse step already gathered them"""
        if n_probe_list is None:
            n_probe_list = torch.full((x.shape[1],), cells.shape[1], device=self.device, dtype=torch.long)
        cell_start, cell_size = (self._cell_start[cells], self._cell_size[cells]) if extents is None else extents
        # expected slots per query (host-side estimate, no sync): bounds the per-query split
        slots_hint = cells.shape[1] * self.capacity // max(self.n_cells, 1)
        return n_probe_list, cell_start, cell_size, slots_hint, self._is_empty if self._has_holes else None

    def _search_batches(self, x, per_batch, alongside=()):
        """search() over batches of `max_query_batch` prepared queries: per_batch(xb, sims, cells, n_probe_list,
        extents) returns a tuple of [n_batch, k] tensors; the concatenations (a single batch's own tensors).
        `alongside`: per-query tensors [n_query, ...] (or None) that are cut as the queries are and handed to
        per_batch behind xb -- a filtered search's row of every query"""
        out = []
        for q0 in range(0, max(x.shape[1], 1), self.max_query_batch):
            xb = x[:, q0:q0 + self.max_query_batch].contiguous()
            cut = tuple(None if t is None else t[q0:q0 + self.max_query_batch].contiguous() for t in alongside)
            out.append(per_batch(xb, *cut, *self._probe_with_extents(xb)))
        return out[0] if len(out) == 1 else tuple(torch.cat(t, 0) for t in zip(*out))

    @property
    def use_smart_probing(self):
        return self._use_smart_probing

    @use_smart_probing.setter
    def use_smart_probing(self, value):
        assert type(value) is bool
        self._use_smart_probing = value

    @property
    def smart_probing_temperature(self):
        return self._smart_probing_temperature

    @smart_probing_temperature.setter
    def smart_probing_temperature(self, value):
        assert value > 0
        assert self.use_smart_probing, "set use_smart_probing to True first"
        self._smart_probing_temperature = value

    def _probe_with_extents(self, x):
        """probe() plus the (start, size) of every probed cell, or None when not gathered"""
        if self.use_fused_probe and self.use_cublas and self.n_probe <= 1024:
            smart = self.use_smart_probing and self.n_probe > 1
            sims, cells, cs, sz, npl = self._coarse_probe(
                x, self.vq_codec.codebook, self._cell_start, self._cell_size, self.n_probe,
                self.smart_probing_temperature if smart else None, prepared=self._probe_prepared())
            return sims, cells, npl, (cs, sz)
        return (*self.probe(x), None)

    def _probe_prepared(self):
        """the coarse codebook's share of the fp16 selection pass, rebuilt when the codebook changes"""
        cb = self.vq_codec.codebook
        key = (cb.data_ptr(), tuple(cb.shape), util.tensor_version(cb))
        cached = getattr(self, "_probe_prep_cache", None)
        # (the entry HOLDS the codebook tensor and is matched by identity: a later codebook allocated at the freed
        # address with the same shape and version -- train, search, train, train, search -- must not hit it)
        if cached is None or cached[0] != key or cached[2] is not cb or cb.is_inference():
            self._probe_prep_cache = cached = (key, self._coarse_probe.prepare(cb), cb)
        return cached[1]

    def probe(self, x):
        """Coarse step: (topk_sims, cells [n_query, n_probe], n_probe_list [n_query])."""
        if self.use_fused_probe and self.use_cublas and self.n_probe <= 1024:
            return self._probe_with_extents(x)[:3]
        vq_codebook = self.vq_codec.codebook
        if self.use_cublas and self.n_probe <= 1024:
            # library GEMM, then the 2ab - a^2 - b^2 epilogue (reference rounding order) fused into
            # the row select: one pass over the [n_query, n_cells] matrix instead of four
            dots = x.transpose(0, 1).contiguous() @ vq_codebook
            topk_sims, cells = self._coarse_select(dots, (x * x).sum(dim=0),
                                                   (vq_codebook * vq_codebook).sum(dim=0), self.n_probe)
        elif self.use_cublas:
            sims = metric.negative_squared_l2_distance(x, vq_codebook).contiguous()
            topk_sims, cells = self._topk(sims, k=self.n_probe, dim=1)
        else:
            topk_sims, cells = self.vq_codec.kmeans.topk(x, k=self.n_probe)
        if self.use_smart_probing and self.n_probe > 1:
            n_probe_list = self._smart_probing(topk_sims, self.smart_probing_temperature)
        else:
            n_probe_list = torch.full((x.shape[1],), self.n_probe, device=self.device,
                                      dtype=torch.long)
        return topk_sims, cells, n_probe_list
