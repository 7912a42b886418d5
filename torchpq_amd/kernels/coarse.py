"""The coarse step of a search: row top-k, the fused epilogue + select, the one-call probe, smart probing."""
import torch

from .. import _lib
from .._lib import load, ptr, require_gpu
from ._common import alloc_pair, call


class TopkSelectHip:
    """Row-wise top-k, values descending (kernels/TopkSelectCuda.py:52-84,
    Top32SelectCuda.py:60-112, Top1SelectCuda.py)."""

    def __init__(self, tpb=256, queue_capacity=4, buffer_size=4):
        self.tpb = tpb

    def __call__(self, x, k=1, dim=1):
        assert len(x.shape) == 2
        assert dim in (1, -1), "only support last dimention"
        assert x.dtype == torch.float32
        assert 1 <= k <= 1024 and k <= x.shape[1]
        x = x.contiguous()
        require_gpu(x)
        rows, cols = x.shape
        vals, inds = alloc_pair(rows, k, x.device)
        call("tpq_topk_select", x.device, ptr(x), ptr(vals), ptr(inds), rows, cols, k)
        return vals, inds


class CoarseSelectHip:
    """negative_squared_l2_distance epilogue + row top-k in one pass (metric.py:89-96 + fn/Topk.py):
    dots [n_query, n_cells] = x^T C, a2 [n_query], b2 [n_cells] -> (sims, cells) [n_query, k]."""

    def __call__(self, dots, a2, b2, k):
        assert dots.dtype == a2.dtype == b2.dtype == torch.float32 and len(dots.shape) == 2
        rows, cols = dots.shape
        assert a2.shape == (rows,) and b2.shape == (cols,)
        assert 1 <= k <= 1024 and k <= cols
        dots, a2, b2 = dots.contiguous(), a2.contiguous(), b2.contiguous()
        require_gpu(dots, a2, b2)
        vals, inds = alloc_pair(rows, k, dots.device)
        call("tpq_coarse_select", dots.device, ptr(dots), ptr(a2), ptr(b2), ptr(vals), ptr(inds), rows, cols, k)
        return vals, inds


Top1SelectHip = TopkSelectHip
Top32SelectHip = TopkSelectHip


class CoarseProbeHip:
    """The coarse step of IVFPQIndex.search in one call (tpq_ivfpq_coarse_probe): sims on the fp32
    matrix cores, row top-n_probe, list extents of the chosen cells, per-query probe count."""

    ROUTES = {"auto": _lib.PROBE_ROUTE_AUTO, "fp32": _lib.PROBE_ROUTE_FP32, "fp16": _lib.PROBE_ROUTE_FP16}

    def __init__(self, route="auto"):
        """route: which arithmetic SELECTS ("auto": the library's thresholds; "fp32": the fp32-MFMA kernels;
        "fp16": the fp16 selection pass + exact candidates wherever the shape allows) -- the result is the
        same, bit for bit, on every route (tpq_ivfpq_coarse_probe_route)"""
        assert route in self.ROUTES
        self.route = route

    @staticmethod
    def prepare(centroids):
        """the centroid-only part of the fp16 selection pass (tpq_ivfpq_coarse_probe_prepare), or None when the
        shape has none: a uint8 tensor to pass as `prepared` for as long as `centroids` does not change"""
        d, n_cells = centroids.shape
        assert centroids.dtype == torch.float32
        centroids = centroids.contiguous()
        require_gpu(centroids)
        nbytes = load().tpq_ivfpq_coarse_probe_prepared_bytes(d, n_cells)
        if nbytes == 0:
            return None
        out = torch.empty(nbytes, device=centroids.device, dtype=torch.uint8)
        call("tpq_ivfpq_coarse_probe_prepare", centroids.device, ptr(centroids), d, n_cells, ptr(out), nbytes)
        return out

    def __call__(self, query, centroids, cell_start, cell_size, n_probe, smart_temperature=None, prepared=None):
        """query [d, n_query] f32, centroids [d, n_cells] f32, cell_start / cell_size [n_cells] i64
        -> (topk_sims [n_query, n_probe] f32, cells, cell_start, cell_size [n_query, n_probe] i64,
            n_probe_list [n_query] i64)"""
        d, nq = query.shape
        n_cells = centroids.shape[1]
        assert centroids.shape[0] == d and query.dtype == centroids.dtype == torch.float32
        assert cell_start.shape == cell_size.shape == (n_cells,)
        assert cell_start.dtype == cell_size.dtype == torch.int64
        assert 1 <= n_probe <= min(n_cells, 1024)
        query = query.contiguous()
        centroids = centroids.contiguous()
        require_gpu(query, centroids, cell_start, cell_size)
        dev = query.device
        sims, cells = alloc_pair(nq, n_probe, dev)
        cs = torch.empty(nq, n_probe, device=dev, dtype=torch.int64)
        sz = torch.empty(nq, n_probe, device=dev, dtype=torch.int64)
        npl = torch.empty(nq, device=dev, dtype=torch.int64)
        if nq == 0:
            return sims, cells, cs, sz, npl
        route = self.ROUTES[self.route]
        ws_bytes = load().tpq_ivfpq_coarse_probe_route_workspace_bytes(d, nq, n_cells, route)
        ws = torch.empty(ws_bytes, device=dev, dtype=torch.uint8)
        t = float(smart_temperature) if smart_temperature else 0.0
        call("tpq_ivfpq_coarse_probe_route", dev,
             ptr(query), ptr(centroids), ptr(cell_start), ptr(cell_size), ptr(sims), ptr(cells),
             ptr(cs), ptr(sz), ptr(npl), d, nq, n_cells, n_probe, t, route, ptr(prepared), ptr(ws), ws_bytes)
        return sims, cells, cs, sz, npl


class SmartProbingHip:
    """n_probe_list from the entropy of the coarse similarities (index/IVFPQIndex.py:499-512)."""

    def __call__(self, topk_sims, temperature=30.0):
        assert topk_sims.dtype == torch.float32 and len(topk_sims.shape) == 2
        topk_sims = topk_sims.contiguous()
        require_gpu(topk_sims)
        rows, n_probe = topk_sims.shape
        out = torch.empty(rows, device=topk_sims.device, dtype=torch.int64)
        call("tpq_smart_probing", topk_sims.device, ptr(topk_sims), ptr(out), rows, n_probe, float(temperature))
        return out
