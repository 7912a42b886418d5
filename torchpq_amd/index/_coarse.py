"""The coarse step of the IVF indexes (IVFPQIndex and its subclasses, IVFFlatIndex): the probed cells of a query batch.

The host class provides `vq_codec` (a trained VQCodec), `n_probe`, `device`, the container's `_cell_start` /
`_cell_size`, the switches `use_cublas` and `use_fused_probe`, `_use_smart_probing` / `_smart_probing_temperature`,
and the kernel wrappers `_coarse_probe`, `_coarse_select`, `_topk`, `_smart_probing`.
"""
import torch

from .. import metric, util


class CoarseProbeMixin:
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
