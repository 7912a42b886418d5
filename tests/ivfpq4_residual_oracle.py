"""NumPy oracle of the IVFPQ4Index list scan over residual codes (tpq_ivfpq4_scan_residual_topk; reconstruction, table
entry, value and order: include/torchpq_amd.h).

float32 throughout, as tests/ivfpq4_oracle.py: a table entry is accumulated in ONE loop over the sub-vector's
dimensions (the reconstruction centroid + codeword is one add of its own, then a difference and a product, or a
product, then a sum: no fused multiply-add), a slot's value in ONE loop over the sub-quantizers.  The tables are per
(query, probe): a slot is valued under the probe that scans it.  Candidates, the skipped duplicate probe, the cut at
the storage, order and padding are those of tests/ivfpq4_oracle.py (`probed_slots` on one probe at a time, the same
lexsort).
"""
import numpy as np

from ivfpq4_oracle import probed_slots, unpack


def lut(query, codebook, centroids, cells, distance="euclidean"):
    """query f32 [d, nq], codebook f32 [m, ds, 16], centroids f32 [n_cells, d], cells i64 [nq, n_probe] -> the tables
    f32 [nq, n_probe, m, 16]"""
    m, ds, kk = codebook.shape
    assert kk == 16 and query.shape[0] == m * ds and centroids.shape[1] == m * ds
    nq, n_probe = cells.shape
    q = np.ascontiguousarray(query.astype(np.float32).T).reshape(nq, 1, m, ds)
    cen = centroids.astype(np.float32)[cells].reshape(nq, n_probe, m, ds)
    cb = codebook.astype(np.float32)
    e = np.zeros((nq, n_probe, m, 16), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(ds):
            y = cen[:, :, :, i, None] + cb[None, None, :, i, :]        # the reconstruction: one add
            x = q[:, :, :, i, None]
            if distance == "euclidean":
                t = x - y
                e = e - t * t
            else:
                e = e + x * y
    assert e.dtype == np.float32
    return e


def values(table, codes, qi, pi, slots):
    """table f32 [nq, n_probe, m, 16], codes u8 [m, capacity]; qi, pi, slots [n]: the value of slot slots[i] for query
    qi[i] under probe pi[i] -> f32 [n]"""
    m = table.shape[2]
    v = np.zeros(len(slots), np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(m):
            v = v + table[qi, pi, j, codes[j, slots]]
    assert v.dtype == np.float32
    return v


def probe_slots(cell_start, cell_size, n_probe, capacity):
    """one query: (the probe of every scanned slot, the scanned slots) in scan order -- probed_slots, probe by probe
    (a duplicate probe scans nothing)"""
    n_probe = int(min(max(int(n_probe), 0), len(cell_start)))
    ps, ss = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for p in range(n_probe):
        if p > 0 and cell_start[p] == cell_start[p - 1]:
            continue
        s = probed_slots(cell_start[p:p + 1], cell_size[p:p + 1], 1, capacity)
        ps.append(np.full(len(s), p, np.int64))
        ss.append(s)
    return np.concatenate(ps), np.concatenate(ss)


def scan_topk(storage, query, codebook, centroids, cells, is_empty, cell_start, cell_size, n_probe_list, k,
              distance="euclidean"):
    """storage u8 [m / 8, capacity, 4], query f32 [d, nq], codebook f32 [m, ds, 16], centroids f32 [n_cells, d],
    cells / cell_start / cell_size i64 [nq, max_nprobe], is_empty u8 [capacity] or None, n_probe_list i64 [nq]
    -> (values f32 [nq, k], address i64 [nq, k])"""
    codes = unpack(storage)
    capacity = codes.shape[1]
    nq = query.shape[1]
    out_v = np.full((nq, k), -np.inf, np.float32)
    out_a = np.full((nq, k), -1, np.int64)
    step = 64                                          # (blocks of queries: the tables of a block at once)
    for q0 in range(0, nq, step):
        qs = range(q0, min(q0 + step, nq))
        table = lut(query[:, q0:q0 + step], codebook, centroids, cells[q0:q0 + step], distance)
        per_query = [probe_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity) for q in qs]
        if is_empty is not None:
            per_query = [(p[is_empty[s] == 0], s[is_empty[s] == 0]) for p, s in per_query]
        qi = np.concatenate([np.full(len(s), q - q0, np.int64) for q, (_, s) in zip(qs, per_query)])
        vals_all = values(table, codes, qi, np.concatenate([p for p, _ in per_query]),
                          np.concatenate([s for _, s in per_query]))
        for q, (_, s) in zip(qs, per_query):
            v = vals_all[qi == q - q0]
            keep = ~np.isnan(v)
            s, v = s[keep], v[keep]
            order = np.lexsort((s, -v.astype(np.float64)))[:k]
            out_v[q, :len(order)] = v[order]
            out_a[q, :len(order)] = s[order]
    return out_v, out_a


def search(query, codebook, centroids, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, k,
           distance="euclidean"):
    """IVFPQ4Index(pq_use_residual=True).search on the index's own state and the cells its coarse step returned (query
    already normalised for "cosine"; centroids [n_cells, d]): (values, ids, address)"""
    v, a = scan_topk(storage, query, codebook, centroids, cells, is_empty, cell_start[cells], cell_size[cells],
                     n_probe_list, k, "euclidean" if distance == "euclidean" else "inner")
    ids = np.where(a >= 0, address2id[np.maximum(a, 0)], -1)
    return v, ids, a
