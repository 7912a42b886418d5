"""NumPy oracle of IVFPQ4Index range search (tpq_ivfpq4_range_count / _fill and their residual forms; semantics:
include/torchpq_amd.h), built on the top-k oracles: the codes, table and value of tests/ivfpq4_oracle.py (`unpack`,
`lut`, `values`) for plain codes, the per-probe tables, probe walk and value of tests/ivfpq4_residual_oracle.py (`lut`,
`probe_slots`, `values`) for residual codes.  What this file adds is the order -- the candidates are kept in scan order
-- the optional filter row per query, and the threshold.

A hit of query q is a candidate of the top-k scan -- a slot of its first n_probe_list[q] probed cells (clamped to
[0, max_nprobe]; a probe whose start equals the previous probe's start is skipped), inside the storage, not tombstoned,
allowed by the query's filter row when there is one (a row outside [0, n_filters) allows nothing) -- whose value is
>= threshold[q]; a NaN value or a NaN threshold fails the compare.  Hits come in scan order: probe rank ascending,
then address ascending; a slot of two overlapping cells appears once per probe that scans it.
"""
import numpy as np

import ivfpq4_oracle as porc
import ivfpq4_residual_oracle as rorc
from ivfpq_range_oracle import hits, sort_segments  # noqa: F401  (the threshold and the sort are the 8-bit index's)

F32 = np.float32


def _allowed_row(allowed, rows, q, capacity):
    """bool [capacity]: what query q's row allows; no filter: everything"""
    if allowed is None:
        return np.ones(capacity, bool)
    allowed = np.atleast_2d(np.asarray(allowed, bool))
    row = 0 if rows is None else int(rows[q])
    return allowed[row] if 0 <= row < allowed.shape[0] else np.zeros(capacity, bool)


def candidates(storage, query, codebook, is_empty, cell_start, cell_size, n_probe_list, distance="euclidean",
               centroids=None, cells=None, allowed=None, rows=None, probes=False):
    """per query (slots i64, values f32[, probe ranks i64 with `probes`]) of its live (and allowed) candidates, in
    scan order.
    storage u8 [m / 8, capacity, 4], query f32 [d, nq], codebook f32 [m, ds, 16], is_empty u8 [capacity] or None,
    cell_start / cell_size i64 [nq, max_nprobe], n_probe_list i64 [nq]; residual codes when `centroids` [n_cells, d] and
    `cells` i64 [nq, max_nprobe] are given; allowed bool [n_filters, capacity] or None, rows i32 [nq] or None (row 0)"""
    codes = porc.unpack(storage)
    capacity = codes.shape[1]
    nq = query.shape[1]
    out = []
    step = 64                                          # (blocks of queries: the residual tables of a block at once)
    for q0 in range(0, nq, step):
        qs = range(q0, min(q0 + step, nq))
        if centroids is None:
            table = porc.lut(query[:, q0:q0 + step], codebook, distance)
        else:
            table = rorc.lut(query[:, q0:q0 + step], codebook, centroids, cells[q0:q0 + step], distance)
        for q in qs:
            p, s = rorc.probe_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity)
            keep = _allowed_row(allowed, rows, q, capacity)[s]
            if is_empty is not None:
                keep &= is_empty[s] == 0
            p, s = p[keep], s[keep]
            if centroids is None:
                v = porc.values(table[q - q0:q - q0 + 1], codes, s)[0]
            else:
                v = rorc.values(table, codes, np.full(len(s), q - q0, np.int64), p, s)
            out.append((s.astype(np.int64), v.astype(F32)) + ((p.astype(np.int64),) if probes else ()))
    return out


def range_scan(storage, query, codebook, is_empty, cell_start, cell_size, n_probe_list, threshold,
               distance="euclidean", centroids=None, cells=None, allowed=None, rows=None, cand=None):
    """tpq_ivfpq4_range_count + _fill (or their residual forms): (lims, values, address).  `cand`: what candidates()
    returned for the same inputs, when several thresholds are applied to them (the values are computed once)"""
    if cand is None:
        cand = candidates(storage, query, codebook, is_empty, cell_start, cell_size, n_probe_list, distance,
                          centroids, cells, allowed, rows)
    return hits(cand, threshold)


def range_search(query, codebook, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, threshold,
                 distance="euclidean", centroids=None, id_sets=None, rows=None):
    """IVFPQ4Index.range_search / range_search_filtered on the index's own state and the cells its coarse step returned
    (query already normalised for "cosine"; centroids [n_cells, d] with pq_use_residual; id_sets: the filter's id sets,
    a row allows the slots whose id is in its set): (lims, values, ids, address)"""
    allowed = None
    if id_sets is not None:
        allowed = np.stack([(address2id >= 0) & np.isin(address2id, np.asarray(ids, np.int64)) for ids in id_sets])
    lims, v, a = range_scan(storage, query, codebook, is_empty, cell_start[cells], cell_size[cells], n_probe_list,
                            threshold, "euclidean" if distance == "euclidean" else "inner", centroids=centroids,
                            cells=None if centroids is None else cells, allowed=allowed, rows=rows)
    return lims, v, address2id[a], a
