"""K-means: the assign kernels (exact, split, selecting), the fused Lloyd step, the centroid update."""
import torch

from .. import _lib
from .._lib import load, ptr, require_gpu
from ._common import alloc_pair, call, metric_code


class MaxSimHip:
    """Batched arg-max similarity, mode "tn" (kernels/MaxSimCuda.py:296-340): A [l, d, m] or
    [d, m], B [l, d, n] or [d, n] -> (vals, inds) over the n columns of B.

    precision="fp32" (default): tpq_max_sim, ascending-k fp32 fma chains on the fp32 MFMA,
    bit-exact against the oracle -- the encode / predict path.
    precision="bf16x3": tpq_max_sim_split, exact 3-way bf16 split of both operands on the bf16
    matrix cores (fp32-level accuracy, different rounding points; near-ties may resolve
    differently) -- the Lloyd loop of MultiKMeans.fit; shapes it does not cover fall back to the
    fp32 kernel (`split_supported`)."""

    def __init__(self, dim=2, distance="euclidean", precision="fp32", **_):
        assert distance in ("euclidean", "inner", "cosine")
        assert precision in ("fp32", "bf16x3")
        self.distance = distance
        self.dim = dim
        self.precision = precision

    @staticmethod
    def split_supported(d, m, n):
        return bool(load().tpq_max_sim_split_supported(int(d), int(m), int(n)))

    def __call__(self, A, B, dim=1, mode="tn"):
        assert mode == "tn", "only the 'tn' layout ([.., d, m] x [.., d, n]) is on the IVFPQ path"
        assert len(A.shape) == len(B.shape)
        two_d = len(A.shape) == 2
        if two_d:
            A, B, dim = A[None], B[None], dim + 1
        assert len(A.shape) == 3
        assert dim == 2, "arg-max is taken over the columns of B (dim=2; dim=1 for 2-D inputs)"
        assert A.shape[0] == B.shape[0] and A.shape[1] == B.shape[1]
        assert A.dtype == B.dtype == torch.float32
        A = A.contiguous()
        B = B.contiguous()
        require_gpu(A, B)
        l, d, m = A.shape
        n = B.shape[2]
        vals, inds = alloc_pair(l, m, A.device)
        split = self.precision == "bf16x3" and self.split_supported(d, m, n)
        call("tpq_max_sim_split" if split else "tpq_max_sim", A.device,
             ptr(A), ptr(B), ptr(vals), ptr(inds), l, d, m, n, metric_code(self.distance))
        if two_d:
            vals, inds = vals[0], inds[0]
        return vals, inds


class CoarseAssignHip:
    """Labels of MaxSimHip (fp32), bit for bit, for ONE problem with many centroids -- the coarse
    assign of IVFPQIndex.add / VQCodec.encode (kernels/MaxSimCuda.py:296-340 as called from
    clustering/KMeans.py:440-452): A [d, m], B [d, n] -> labels [m] int64, d <= 1024.  Error-bounded
    top-2 selection on the matrix cores; the points it leaves undecided get the exact kernel's own
    value -- over all centroids, or (from 4 096 centroids on, and for d > 128) for each of their
    candidates, the 2-3 centroids within twice the bound of the best (tpq_coarse_assign)."""

    # "auto": the library's size thresholds pick the path; "cascade": the fp16 cascade for every shape it
    # supports (tpq_coarse_assign_route; the parity tests set this to drive the cascade over small shapes)
    default_route = "auto"

    def __init__(self, distance="euclidean", route=None, **_):
        assert distance in ("euclidean", "inner", "cosine")
        assert route in (None, "auto", "cascade")
        self.distance = distance
        self.route = route
        self._last = None

    @staticmethod
    def supported(d, m, n):
        return bool(load().tpq_coarse_assign_supported(int(d), int(m), int(n)))

    def __call__(self, A, B, return_vals=False):
        """labels [m]; return_vals=True: (vals, labels) with vals the maximum similarity, approximate
        (within the selection bound) except for re-checked points"""
        assert A.dim() == 2 and B.dim() == 2 and A.shape[0] == B.shape[0]
        assert A.dtype == B.dtype == torch.float32
        A = A.contiguous()
        B = B.contiguous()
        require_gpu(A, B)
        d, m = A.shape
        n = B.shape[1]
        lib = load()
        inds = torch.empty(m, device=A.device, dtype=torch.int64)
        if m == 0:  # (empty tensors have null data pointers)
            self._last = None
            return (torch.empty(0, device=A.device), inds) if return_vals else inds
        route = (_lib.ASSIGN_ROUTE_CASCADE if (self.route or self.default_route) == "cascade"
                 else _lib.ASSIGN_ROUTE_AUTO)
        ws_bytes = lib.tpq_coarse_assign_route_workspace_bytes(d, m, n, route)
        ws = torch.empty(max(ws_bytes, 1), device=A.device, dtype=torch.uint8)
        vals = torch.empty(m, device=A.device, dtype=torch.float32) if return_vals else None
        call("tpq_coarse_assign_route", A.device, ptr(A), ptr(B), ptr(vals), ptr(inds), d, m, n,
             metric_code(self.distance), route, ptr(ws), ws_bytes)
        self._last = (ws, lib.tpq_coarse_assign_count_offset(d, m, n))
        return (vals, inds) if return_vals else inds

    def last_rechecked(self):
        """diagnostics (synchronises): points of the last call that took an exact step (the exact kernel, or
        exact values of their candidates)"""
        if self._last is None:
            return 0
        ws, off = self._last
        return int(ws[off:off + 4].view(torch.int32).item())


class MaxSimSelectHip:
    """(vals, labels) for l codebook-sized problems (n <= 256 centroids, d <= 64): A [l, d, m], B [l, d, n].
    Labels are MaxSimHip's (fp32), bit for bit; vals are the selection's fast maxima, exact only for
    re-checked points (tpq_max_sim_select: bounded bf16 top-2 selection + exact re-check)."""

    def __init__(self, distance="euclidean", **_):
        assert distance in ("euclidean", "inner", "cosine")
        self.distance = distance
        self._ws = None

    @staticmethod
    def supported(l, d, m, n):
        return bool(load().tpq_max_sim_select_supported(int(l), int(d), int(m), int(n)))

    def __call__(self, A, B):
        assert A.dim() == 3 and B.dim() == 3 and A.shape[:2] == B.shape[:2]
        assert A.dtype == B.dtype == torch.float32
        A = A.contiguous()
        B = B.contiguous()
        require_gpu(A, B)
        l, d, m = A.shape
        n = B.shape[2]
        vals, inds = alloc_pair(l, m, A.device)
        if m == 0:
            return vals, inds
        ws_bytes = load().tpq_max_sim_select_workspace_bytes(l, d, m, n)
        if self._ws is None or self._ws.numel() < ws_bytes or self._ws.device != A.device:
            self._ws = None
            self._ws = torch.empty(max(ws_bytes, 1), device=A.device, dtype=torch.uint8)
        call("tpq_max_sim_select", A.device, ptr(A), ptr(B), ptr(vals), ptr(inds), l, d, m, n,
             metric_code(self.distance), ptr(self._ws), ws_bytes)
        return vals, inds

    def release(self):
        """drop the cached workspace (l x m int32 lists)"""
        self._ws = None


class LloydStepHip:
    """One Lloyd iteration of MultiKMeans.fit on prepared data (tpq_lloyd_prepare / tpq_lloyd_step):
    the get_labels -> compute_centroids pair of the reference's driver
    (torchpq/clustering/MultiKMeans.py:415-453) for codebook-sized euclidean problems.

        step = LloydStepHip(data, centroids0)       # once per fit: centre, scale, split, fragment order
        maxsims, labels, new_centroids = step(centroids)

    labels are MaxSimHip's (fp32), bit for bit; maxsims are the selection's fast maxima (exact for
    re-checked points); new_centroids are the means of the labelled points summed from the fp16 pieces (h + m, two
    ulps of fp32 per element): within ~2e-7 of the scale of ComputeCentroidsHip()(data, labels, k), not bit-equal --
    a fit() that takes this path (MultiKMeans.lloyd_min_work / lloyd_min_iter) and one that does not agree to that
    tolerance per iteration."""

    @staticmethod
    def supported(l, d, m, n):
        return bool(load().tpq_lloyd_supported(int(l), int(d), int(m), int(n)))

    def __init__(self, data, centroids0):
        assert data.dim() == 3 and centroids0.dim() == 3 and data.shape[:2] == centroids0.shape[:2]
        assert data.dtype == centroids0.dtype == torch.float32
        require_gpu(data, centroids0)
        self.data = data.contiguous()
        centroids0 = centroids0.contiguous()
        l, d, m = self.data.shape
        n = centroids0.shape[2]
        assert self.supported(l, d, m, n), "shape not supported by tpq_lloyd_step (d <= 64, n <= 256)"
        self.shape = (l, d, m, n)
        lib = load()
        nbytes = lib.tpq_lloyd_prepared_bytes(l, d, m)
        self.prepared = torch.empty(nbytes, device=data.device, dtype=torch.uint8)
        # the step workspace (two l x m int lists, the sums) is allocated HERE, with the prepared copy: a caller
        # that guards the construction against torch.cuda.OutOfMemoryError (MultiKMeans.fit) then never meets one
        # inside its Lloyd loop
        self._ws = torch.empty(max(lib.tpq_lloyd_step_workspace_bytes(l, d, m, n), 1), device=data.device,
                               dtype=torch.uint8)
        call("tpq_lloyd_prepare", data.device, ptr(self.data), ptr(centroids0), ptr(self.prepared), nbytes,
             l, d, m, n)

    def __call__(self, centroids, update=True):
        l, d, m, n = self.shape
        assert tuple(centroids.shape) == (l, d, n) and centroids.dtype == torch.float32
        centroids = centroids.contiguous()
        require_gpu(centroids)
        dev = self.data.device
        vals, inds = alloc_pair(l, m, dev)
        new = torch.empty(l, d, n, device=dev, dtype=torch.float32) if update else None
        ws_bytes = load().tpq_lloyd_step_workspace_bytes(l, d, m, n)
        if self._ws is None or self._ws.numel() < ws_bytes:
            self._ws = None
            self._ws = torch.empty(max(ws_bytes, 1), device=dev, dtype=torch.uint8)
        call("tpq_lloyd_step", dev, ptr(self.data), ptr(self.prepared), ptr(centroids), ptr(new), ptr(vals),
             ptr(inds), l, d, m, n, ptr(self._ws), ws_bytes)
        return vals, inds, new

    def rechecked(self, level=2):
        """points per sub-problem the last step left undecided after level 1 (coarse pass) or level 2
        (= sent to the exact fp32 re-check); int32 [l], diagnostics"""
        l, d, m, n = self.shape
        off = load().tpq_lloyd_step_count_offset(l, d, m, n, int(level))
        return self._ws[off:off + 4 * l].view(torch.int32).clone()


class ComputeCentroidsHip:
    """K-means update (kernels/ComputeCentroidsCuda.py:43-81): data [l, d, n], labels [l, n]
    -> centroids [l, d, k]; empty clusters -> 0."""

    def __init__(self, de=1, dk=None, sm_size=None, **_):
        pass

    def __call__(self, data, labels, k, centroids=None):
        l, d, n = data.shape
        assert labels.shape == (l, n)
        assert data.dtype == torch.float32 and labels.dtype == torch.int64
        data = data.contiguous()
        labels = labels.contiguous()
        require_gpu(data, labels)
        out = torch.empty(l, d, k, device=data.device, dtype=torch.float32)
        ws_bytes = load().tpq_compute_centroids_workspace_bytes(l, d, k)
        ws = torch.empty(ws_bytes, device=data.device, dtype=torch.uint8)
        call("tpq_compute_centroids", data.device, ptr(data), ptr(labels), ptr(out), l, d, n, k, ptr(ws), ws_bytes)
        return out
