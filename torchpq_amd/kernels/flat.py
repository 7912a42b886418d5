"""Exact search without its similarity matrix: the fused fp32-MFMA similarity + top-k of FlatIndex."""
import torch

from .._lib import load, ptr, require_gpu
from ._common import alloc_topk, call, metric_code

CHUNK = 256          # slots per chunk of the tile kernel (kCsRows, csrc/sims_chunk.h)
QUERY_BLOCK = 128    # queries per workgroup


def flat_parts(n_query, n_slots, n_cus):
    """Slot ranges per query (n_parts of tpq_flat_topk).  The tile kernel's LDS (its 128 per-query queues) admits one
    workgroup per CU, so the grid -- ceil(n_query / 128) x n_parts workgroups -- should come close to a whole number of
    rounds over the CUs: the fewest parts that fill >= 85 % of their rounds (every further part is one more list per
    query to warm up and to merge), else the best filling among up to two rounds' worth; at least one chunk per part."""
    groups = -(-n_query // QUERY_BLOCK)
    chunks = max(1, -(-n_slots // CHUNK))
    most = max(1, min(1024, chunks, (2 * n_cus) // groups))
    best, best_fill = 1, 0.0
    for parts in range(1, most + 1):
        blocks = groups * parts
        fill = blocks / (-(-blocks // n_cus) * n_cus)
        if fill >= 0.85:
            return parts
        if fill > best_fill:
            best, best_fill = parts, fill
    return best


class FlatTopkHip:
    """tpq_flat_topk (csrc/flat_topk.hip): the k best stored vectors of every query, selected in the epilogue of the
    similarity tiles -- nothing of size [n_query, n_slots] is allocated.  Value and order are defined in
    include/torchpq_amd.h; the result does not depend on n_parts."""

    def __init__(self):
        self.n_cus = None
        self.last_n_parts = None   # diagnostics / tests: slot ranges per query of the last call

    def __call__(self, vectors, query, k, address2id=None, distance="euclidean", n_parts=None):
        """
          vectors: [d, n_slots] float32 (or [d, n_slots, 1]: FlatIndex._storage)
          query: [d, n_query] float32 (normalised by the caller for "cosine")
          address2id: [n_slots] int64 or None; a slot is live iff its entry is >= 0 (None: every slot)
        returns (values [n_query, k] descending, address [n_query, k], ids [n_query, k] or None);
        unfilled = (-inf, -1, -1)
        """
        if vectors.dim() == 3:
            assert vectors.shape[2] == 1
            vectors = vectors[:, :, 0]
        d, n_slots = vectors.shape
        assert query.dim() == 2 and query.shape[0] == d and d >= 1
        n_query = query.shape[1]
        assert vectors.dtype == query.dtype == torch.float32
        if address2id is not None:
            assert address2id.shape == (n_slots,) and address2id.dtype == torch.int64
        assert distance in ("euclidean", "cosine", "inner")
        assert 0 < k <= 1024
        query = query.contiguous()
        require_gpu(vectors, query, address2id)
        device = vectors.device
        values, address, ids = alloc_topk(n_query, k, device, address2id)
        if n_query == 0:
            return values, address, ids
        if n_parts is None:
            if self.n_cus is None:
                self.n_cus = torch.cuda.get_device_properties(device).multi_processor_count
            n_parts = flat_parts(n_query, n_slots, self.n_cus)
        self.last_n_parts = n_parts
        ws_bytes = load().tpq_flat_topk_workspace_bytes(n_query, k, n_parts)
        ws = torch.empty(ws_bytes, device=device, dtype=torch.uint8)
        call("tpq_flat_topk", device, ptr(vectors), ptr(query), ptr(address2id), ptr(values), ptr(address), ptr(ids),
             n_slots, d, n_query, k, metric_code(distance), n_parts, ptr(ws), ws_bytes)
        return values, address, ids


RANGE_BLOCKS_PER_CU = 2   # workgroups of the range kernels a CU holds (256 registers a lane, 33 KiB of LDS each)
RANGE_ROUNDS = 4          # ... and how many times over the grid should fill them


def flat_range_parts(n_query, n_slots, n_cus):
    """Slot ranges per query (n_parts of tpq_flat_range_count / _fill).  A part costs one counter per query and
    nothing else -- no list to warm up, none to merge -- and the fill pass skips every workgroup whose 128 segments are
    empty, so parts are made fine rather than few: the fewest parts that give RANGE_ROUNDS x RANGE_BLOCKS_PER_CU x n_cus
    workgroups (the grid is ceil(n_query / 128) x n_parts; four rounds keep the last, partly filled round a small share
    of the call), at least one 256-slot chunk per part, at most 1024 parts."""
    groups = -(-n_query // QUERY_BLOCK)
    chunks = max(1, -(-n_slots // CHUNK))
    want = -(-(RANGE_ROUNDS * RANGE_BLOCKS_PER_CU * n_cus) // max(groups, 1))
    return max(1, min(1024, chunks, want))


class FlatRangeHip:
    """tpq_flat_range_count / tpq_flat_range_fill (csrc/flat_range.hip): every live stored vector whose value is >= the
    query's threshold, over the whole database, in address order -- the similarity tiles of FlatTopkHip with a count
    and a fill epilogue; nothing of size [n_query, n_slots] is allocated.  The semantics are defined in
    include/torchpq_amd.h; the result does not depend on n_parts."""

    def __init__(self):
        self.n_cus = None
        self.last_n_parts = None   # diagnostics / tests: slot ranges per query of the last call

    def __call__(self, vectors, query, threshold, address2id=None, distance="euclidean", n_parts=None):
        """
          vectors, query, address2id: as FlatTopkHip
          threshold: a Python float, or [n_query] float32 -- one per query
        returns (lims [n_query + 1] int64, values [total] float32, address [total] int64, ids [total] int64 or None):
        the hits of query q are values[lims[q]:lims[q+1]] / address[lims[q]:lims[q+1]], address ascending.
        Synchronises once: the number of hits sizes the outputs.
        """
        if vectors.dim() == 3:
            assert vectors.shape[2] == 1
            vectors = vectors[:, :, 0]
        d, n_slots = vectors.shape
        assert query.dim() == 2 and query.shape[0] == d and d >= 1
        n_query = query.shape[1]
        assert vectors.dtype == query.dtype == torch.float32
        if address2id is not None:
            assert address2id.shape == (n_slots,) and address2id.dtype == torch.int64
        assert distance in ("euclidean", "cosine", "inner")
        per_query = torch.is_tensor(threshold)
        if per_query:
            assert threshold.shape == (n_query,) and threshold.dtype == torch.float32
            threshold = threshold.contiguous()
        query = query.contiguous()
        require_gpu(vectors, query, address2id, threshold if per_query else None)
        device = vectors.device
        if not per_query:
            threshold = torch.full((n_query,), float(threshold), device=device, dtype=torch.float32)
        if n_query == 0:
            empty = torch.empty(0, device=device, dtype=torch.int64)
            return (torch.zeros(1, device=device, dtype=torch.int64),
                    torch.empty(0, device=device, dtype=torch.float32), empty,
                    None if address2id is None else empty.clone())
        if n_parts is None:
            if self.n_cus is None:
                self.n_cus = torch.cuda.get_device_properties(device).multi_processor_count
            n_parts = flat_range_parts(n_query, n_slots, self.n_cus)
        self.last_n_parts = n_parts
        n_seg = load().tpq_flat_range_segments(n_query, n_parts)
        assert n_seg == n_query * n_parts, (n_query, n_parts)
        inputs = (ptr(vectors), ptr(query), ptr(address2id), ptr(threshold))
        shape = (n_slots, d, n_query, metric_code(distance), n_parts)
        counts = torch.empty(n_seg, device=device, dtype=torch.int32)
        call("tpq_flat_range_count", device, *inputs, ptr(counts), *shape)
        offsets = torch.zeros(n_seg + 1, device=device, dtype=torch.int64)
        offsets[1:] = torch.cumsum(counts, 0, dtype=torch.int64)
        total = int(offsets[-1].item())     # the host sync a variable-size output needs
        values = torch.empty(total, device=device, dtype=torch.float32)
        address = torch.empty(total, device=device, dtype=torch.int64)
        ids = torch.empty(total, device=device, dtype=torch.int64) if address2id is not None else None
        if total:
            call("tpq_flat_range_fill", device, *inputs, ptr(offsets), ptr(values), ptr(address), ptr(ids), *shape)
        return offsets[::n_parts].contiguous(), values, address, ids
