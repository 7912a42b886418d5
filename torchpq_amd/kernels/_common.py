"""What the kernel wrappers share: the library call, the metric code, the output tensors, the per-query split."""
import torch

from .. import _lib
from .._lib import check, load, stream_ptr


def call(name, device, *args):
    """lib.<name>(*args, current stream of `device`) with `device` current; raises on a non-zero return code"""
    with torch.cuda.device(device):
        rc = getattr(load(), name)(*args, stream_ptr(device))
    check(rc, name)


def metric_code(distance):
    """TPQ_METRIC_* of a distance name ("cosine" is the inner product: the caller normalises)"""
    return _lib.METRIC_NEG_SQ_L2 if distance == "euclidean" else _lib.METRIC_INNER


def alloc_pair(rows, cols, device):
    """(float32, int64) outputs of shape [rows, cols]"""
    return (torch.empty(rows, cols, device=device, dtype=torch.float32),
            torch.empty(rows, cols, device=device, dtype=torch.int64))


def alloc_topk(n_query, k, device, address2id):
    """(values, address, ids) of a top-k over slots, [n_query, k]; ids is None without an `address2id`"""
    ids = torch.empty(n_query, k, device=device, dtype=torch.int64) if address2id is not None else None
    return (*alloc_pair(n_query, k, device), ids)


def topk_result(values, address, ids):
    return (values, address) if ids is None else (values, address, ids)


def workgroups_per_query(n_query, n_cus, workgroups_per_cu, waves, slots_hint=None):
    """Workgroups per query so that a small batch still fills the chip with `workgroups_per_cu` workgroups of `waves`
    waves on each CU.  ``slots_hint`` (expected slots scanned per query) caps the split so that every wave still
    walks >= 4 tiles: a wave that sees a single tile admits all 64 slots and the merge drowns."""
    target = workgroups_per_cu * n_cus
    if n_query >= target:
        return 1
    split = max(1, min(64, target // max(n_query, 1)))
    if slots_hint is not None:
        split = max(1, min(split, int(slots_hint) // (64 * waves * 4)))
    return split
