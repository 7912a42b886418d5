"""NumPy oracle of the IVFFlatIndex list scan (tpq_ivfflat_scan_topk; value and order: include/torchpq_amd.h).

float32 throughout.  The value of a slot is accumulated in ONE loop over the dimensions, vectorised across slots
(and queries), so every step rounds as the kernel's does: a product, then a sum, no fused multiply-add.
Candidates of a query: the slots of its first n_probe_list[q] cells (clamped to [0, max_nprobe]; a probe whose start
equals the previous probe's start is skipped), inside the storage, not tombstoned, whose value is not NaN.
Order: value descending, address ascending; positions beyond the candidates are (-inf, -1).
"""
import numpy as np


def as_vectors(storage):
    """CellContainer._storage u8 [d, capacity, 4] -> the stored vectors f32 [d, capacity]"""
    storage = np.ascontiguousarray(storage)
    assert storage.dtype == np.uint8 and storage.shape[2] == 4
    return storage.view(np.float32)[:, :, 0]


def vectors_to_codes(x):
    """f32 [d, n] -> the container's code rows u8 [4 d, n]: row 4 i + b is byte b of component i"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    d, n = x.shape
    return np.ascontiguousarray(x.view(np.uint8).reshape(d, n, 4).transpose(0, 2, 1)).reshape(4 * d, n)


def values(vectors, query, slots, distance="euclidean"):
    """f32 [nq, len(slots)]: the value of every slot of `slots` for every query (query f32 [d, nq])"""
    d, nq = query.shape
    acc = np.zeros((nq, len(slots)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(d):
            x = vectors[i, slots].astype(np.float32)[None, :]
            q = query[i].astype(np.float32)[:, None]
            if distance == "euclidean":
                t = q - x
                acc = acc - t * t
            else:
                acc = acc + q * x
    assert acc.dtype == np.float32
    return acc


def probed_slots(cell_start, cell_size, n_probe, capacity):
    """the slots one query scans, in scan order (a slot of two overlapping cells appears twice, as in the kernel)"""
    out, max_nprobe = [], len(cell_start)
    for p in range(min(max(int(n_probe), 0), max_nprobe)):
        st, sz = int(cell_start[p]), int(cell_size[p])
        if sz <= 0 or (p > 0 and int(cell_start[p - 1]) == st):
            continue
        s = np.arange(st, st + sz, dtype=np.int64)
        out.append(s[(s >= 0) & (s < capacity)])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def scan_topk(vectors, query, is_empty, cell_start, cell_size, n_probe_list, k, distance="euclidean"):
    """vectors f32 [d, capacity], query f32 [d, nq], is_empty u8 [capacity] or None, cell_start / cell_size
    i64 [nq, max_nprobe], n_probe_list i64 [nq] -> (values f32 [nq, k], address i64 [nq, k])"""
    d, capacity = vectors.shape
    nq = query.shape[1]
    per_query = [probed_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity) for q in range(nq)]
    if is_empty is not None:
        per_query = [s[is_empty[s] == 0] for s in per_query]
    union = np.unique(np.concatenate(per_query)) if nq else np.zeros(0, np.int64)
    vals_all = values(vectors, query, union, distance)
    out_v = np.full((nq, k), -np.inf, np.float32)
    out_a = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        s = per_query[q]
        v = vals_all[q, np.searchsorted(union, s)]
        keep = ~np.isnan(v)
        s, v = s[keep], v[keep]
        order = np.lexsort((s, -v.astype(np.float64)))[:k]
        out_v[q, :len(order)] = v[order]
        out_a[q, :len(order)] = s[order]
    return out_v, out_a


def search(query, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, k,
           distance="euclidean"):
    """IVFFlatIndex.search on the index's own state and the cells its coarse step returned (query already
    normalised for "cosine"): (values, ids, address)"""
    v, a = scan_topk(as_vectors(storage), query, is_empty, cell_start[cells], cell_size[cells], n_probe_list, k,
                     distance)
    ids = np.where(a >= 0, address2id[np.maximum(a, 0)], -1)
    return v, ids, a
