"""NumPy oracle of the IVFPQ4Index list scan (tpq_ivfpq4_scan_topk; codes, table entry, value and order:
include/torchpq_amd.h).

float32 throughout.  A table entry is accumulated in ONE loop over the sub-vector's dimensions, vectorised across
centroids and queries, and a slot's value in ONE loop over the sub-quantizers, vectorised across slots and queries,
so every step rounds as the kernel's does: a product, then a sum, no fused multiply-add.
Candidates, order and padding are those of tests/ivfflat_oracle.py (`probed_slots`, the same lexsort).
"""
import numpy as np

from ivfflat_oracle import probed_slots


def unpack(storage):
    """CellContainer._storage u8 [m / 8, capacity, 4] -> the sub-quantizer codes u8 [m, capacity]: byte c of word row
    w holds sub-quantizer 8 w + 2 c in bits 0-3 and 8 w + 2 c + 1 in bits 4-7"""
    storage = np.ascontiguousarray(storage)
    assert storage.dtype == np.uint8 and storage.ndim == 3 and storage.shape[2] == 4
    g, cap, _ = storage.shape
    out = np.empty((g, 4, 2, cap), np.uint8)
    by = storage.transpose(0, 2, 1)          # [g, 4, cap]
    out[:, :, 0] = by & 15
    out[:, :, 1] = by >> 4
    return out.reshape(8 * g, cap)


def pack(codes):
    """u8 [m, n] (values 0 ... 15) -> the container's code rows u8 [m / 2, n]"""
    codes = np.asarray(codes, np.uint8)
    return (codes[0::2] | (codes[1::2] << 4)).astype(np.uint8)


def lut(query, codebook, distance="euclidean"):
    """query f32 [d, nq], codebook f32 [m, ds, 16] -> the tables f32 [nq, m, 16]"""
    m, ds, kk = codebook.shape
    assert kk == 16 and query.shape[0] == m * ds
    nq = query.shape[1]
    q = query.astype(np.float32).reshape(m, ds, nq)
    cb = codebook.astype(np.float32)
    e = np.zeros((nq, m, 16), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(ds):
            x = q[:, i, :].T[:, :, None]          # [nq, m, 1]
            c = cb[None, :, i, :]                 # [1, m, 16]
            if distance == "euclidean":
                t = x - c
                e = e - t * t
            else:
                e = e + x * c
    assert e.dtype == np.float32
    return e


def values(table, codes, slots):
    """table f32 [nq, m, 16], codes u8 [m, capacity] -> f32 [nq, len(slots)]: the value of every slot of `slots`"""
    nq, m, _ = table.shape
    v = np.zeros((nq, len(slots)), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(m):
            v = v + table[:, j, :][:, codes[j, slots]]
    assert v.dtype == np.float32
    return v


def scan_topk(storage, query, codebook, is_empty, cell_start, cell_size, n_probe_list, k, distance="euclidean"):
    """storage u8 [m / 8, capacity, 4], query f32 [d, nq], codebook f32 [m, ds, 16], is_empty u8 [capacity] or None,
    cell_start / cell_size i64 [nq, max_nprobe], n_probe_list i64 [nq] -> (values f32 [nq, k], address i64 [nq, k])"""
    codes = unpack(storage)
    capacity = codes.shape[1]
    nq = query.shape[1]
    per_query = [probed_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity) for q in range(nq)]
    if is_empty is not None:
        per_query = [s[is_empty[s] == 0] for s in per_query]
    union = np.unique(np.concatenate(per_query)) if nq else np.zeros(0, np.int64)
    table = lut(query, codebook, distance)
    out_v = np.full((nq, k), -np.inf, np.float32)
    out_a = np.full((nq, k), -1, np.int64)
    # (blocks of queries: [nq, union] floats at once only while that is small)
    step = max(1, (1 << 24) // max(len(union), 1))
    for q0 in range(0, nq, step):
        vals_all = values(table[q0:q0 + step], codes, union)
        for q in range(q0, min(q0 + step, nq)):
            s = per_query[q]
            v = vals_all[q - q0, np.searchsorted(union, s)]
            keep = ~np.isnan(v)
            s, v = s[keep], v[keep]
            order = np.lexsort((s, -v.astype(np.float64)))[:k]
            out_v[q, :len(order)] = v[order]
            out_a[q, :len(order)] = s[order]
    return out_v, out_a


def search(query, codebook, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, k,
           distance="euclidean"):
    """IVFPQ4Index.search on the index's own state and the cells its coarse step returned (query already normalised
    for "cosine"): (values, ids, address)"""
    v, a = scan_topk(storage, query, codebook, is_empty, cell_start[cells], cell_size[cells], n_probe_list, k,
                     "euclidean" if distance == "euclidean" else "inner")
    ids = np.where(a >= 0, address2id[np.maximum(a, 0)], -1)
    return v, ids, a
