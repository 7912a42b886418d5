"""NumPy oracle of IVFFlatIndex filtered search (IVFFlatIndex.search_filtered / range_search_filtered: the list scan
and the range search of tests/ivfflat_oracle.py and tests/ivfflat_range_oracle.py with, per query, `is_empty |
~allowed[row]` as the mask of slots to skip.  A row outside [0, n_filters) allows nothing; filter_of_query None: row 0.
"""
import numpy as np

import ivfflat_oracle as forc
import ivfflat_range_oracle as rorc
from ivfpq_filtered_oracle import query_masks


def scan_topk(vectors, query, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list, k,
              distance="euclidean"):
    """vectors f32 [d, capacity], query f32 [d, nq], allowed bool [n_filters, capacity], filter_of_query int [nq] or
    None, the rest as ivfflat_oracle.scan_topk -> (values f32 [nq, k], address i64 [nq, k])"""
    nq = query.shape[1]
    out_v = np.full((nq, k), -np.inf, np.float32)
    out_a = np.full((nq, k), -1, np.int64)
    for q, mask in enumerate(query_masks(is_empty, allowed, filter_of_query, nq)):
        out_v[q], out_a[q] = (t[0] for t in forc.scan_topk(vectors, query[:, q:q + 1], mask, cell_start[q:q + 1],
                                                          cell_size[q:q + 1], n_probe_list[q:q + 1], k, distance))
    return out_v, out_a


def candidates(vectors, query, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list,
               distance="euclidean"):
    """per query (slots i64, values f32) of its allowed live candidates, in scan order"""
    nq = query.shape[1]
    out = []
    for q, mask in enumerate(query_masks(is_empty, allowed, filter_of_query, nq)):
        out.extend(rorc.candidates(vectors, query[:, q:q + 1], mask, cell_start[q:q + 1], cell_size[q:q + 1],
                                   n_probe_list[q:q + 1], distance))
    return out


def range_scan(vectors, query, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list, threshold,
               distance="euclidean", cand=None):
    """ivfflat_range_oracle.range_scan over the allowed candidates -> (lims, values, address)"""
    if cand is None:
        cand = candidates(vectors, query, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list,
                          distance)
    return rorc.range_scan(vectors, query, None, cell_start, cell_size, n_probe_list, threshold, distance, cand=cand)


def allowed_rows(address2id, id_sets):
    """a filter row allows the slots whose id is in the set (an id the index does not hold allows nothing)"""
    return np.stack([(address2id >= 0) & np.isin(address2id, np.asarray(ids, np.int64)) for ids in id_sets])


def search_filtered(query, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, id_sets,
                    filter_of_query, k, distance="euclidean"):
    """IVFFlatIndex.search_filtered on the index's own state and the cells its coarse step returned (query already
    normalised for "cosine"), the filter restated from the ids: (values, ids, address)"""
    v, a = scan_topk(forc.as_vectors(storage), query, is_empty, allowed_rows(address2id, id_sets), filter_of_query,
                     cell_start[cells], cell_size[cells], n_probe_list, k, distance)
    return v, np.where(a >= 0, address2id[np.maximum(a, 0)], -1), a


def range_filtered(query, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, id_sets,
                   filter_of_query, threshold, distance="euclidean"):
    """IVFFlatIndex.range_search_filtered likewise: (lims, values, ids, address)"""
    lims, v, a = range_scan(forc.as_vectors(storage), query, is_empty, allowed_rows(address2id, id_sets),
                            filter_of_query, cell_start[cells], cell_size[cells], n_probe_list, threshold, distance)
    return lims, v, address2id[a], a
