"""NumPy oracle of IVFFlatIndex range search (tpq_ivfflat_range_count / tpq_ivfflat_range_fill; semantics:
include/torchpq_amd.h), built on the top-k oracle's candidates and values (tests/ivfflat_oracle.py).

A hit of query q is a candidate of the top-k scan -- a slot of its probed cells, inside the storage, not tombstoned --
whose value is >= threshold[q]; a NaN value or a NaN threshold fails the compare.  Hits come in scan order: probe rank
ascending, then address ascending; a slot of two overlapping cells appears twice.
"""
import numpy as np

import ivfflat_oracle as forc


def candidates(vectors, query, is_empty, cell_start, cell_size, n_probe_list, distance="euclidean"):
    """per query (slots i64, values f32) of its live candidates, in scan order"""
    capacity = vectors.shape[1]
    nq = query.shape[1]
    per_query = [forc.probed_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity) for q in range(nq)]
    if is_empty is not None:
        per_query = [s[is_empty[s] == 0] for s in per_query]
    union = np.unique(np.concatenate(per_query)) if nq else np.zeros(0, np.int64)
    vals_all = forc.values(vectors, query, union, distance)
    return [(s, vals_all[q, np.searchsorted(union, s)]) for q, s in enumerate(per_query)]


def range_scan(vectors, query, is_empty, cell_start, cell_size, n_probe_list, threshold, distance="euclidean",
               cand=None):
    """vectors f32 [d, capacity], query f32 [d, nq], is_empty u8 [capacity] or None, cell_start / cell_size
    i64 [nq, max_nprobe], n_probe_list i64 [nq], threshold a float or f32 [nq]
    -> (lims i64 [nq + 1], values f32 [total], address i64 [total]).  `cand`: what candidates() returned for the same
    inputs, when several thresholds are applied to them (the values are computed once and never changed)"""
    nq = query.shape[1]
    threshold = np.broadcast_to(np.asarray(threshold, np.float32), (nq,))
    lims, vals, adr = np.zeros(nq + 1, np.int64), [], []
    if cand is None:
        cand = candidates(vectors, query, is_empty, cell_start, cell_size, n_probe_list, distance)
    for q, (s, v) in enumerate(cand):
        with np.errstate(invalid="ignore"):
            hit = v >= threshold[q]              # False for a NaN on either side
        vals.append(v[hit])
        adr.append(s[hit])
        lims[q + 1] = lims[q] + int(hit.sum())
    return (lims, np.concatenate(vals).astype(np.float32) if nq else np.zeros(0, np.float32),
            np.concatenate(adr).astype(np.int64) if nq else np.zeros(0, np.int64))


def sort_segments(lims, values, address, *more):
    """each query's segment by (value descending, address ascending): what range_search(sort=True) returns"""
    order = np.concatenate([lo + np.lexsort((address[lo:hi], -values[lo:hi].astype(np.float64)))
                            for lo, hi in zip(lims[:-1], lims[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    return tuple(t[order] for t in (values, address, *more))


def range_search(query, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, threshold,
                 distance="euclidean"):
    """IVFFlatIndex.range_search on the index's own state and the cells its coarse step returned (query already
    normalised for "cosine"): (lims, values, ids, address)"""
    lims, v, a = range_scan(forc.as_vectors(storage), query, is_empty, cell_start[cells], cell_size[cells],
                            n_probe_list, threshold, distance)
    return lims, v, address2id[a], a
