"""NumPy oracle of IVFPQ4Index filtered search (tpq_ivfpq4_scan_filtered_topk / _residual_topk; semantics:
include/torchpq_amd.h): the unfiltered oracles tests/ivfpq4_oracle.scan_topk and tests/ivfpq4_residual_oracle.scan_topk
called with `is_empty | ~allowed[row]` as the tombstone mask -- once per distinct row, every query's line then picked
from the call for its row, so a batch of a thousand queries over five rows is five oracle calls.  A row outside
[0, n_filters) allows nothing.
"""
import numpy as np

import ivfpq4_oracle as porc
import ivfpq4_residual_oracle as rorc
from ivfpq_filtered_oracle import pack_bits, unpack_bits  # noqa: F401  (the bit format is that of the 8-bit index)


def row_mask(is_empty, allowed, row):
    """u8 [capacity]: `is_empty | ~allowed[row]`; no such row: everything is masked"""
    allowed = np.atleast_2d(np.asarray(allowed, bool))
    cap = allowed.shape[1]
    dead = np.zeros(cap, bool) if is_empty is None else np.asarray(is_empty) != 0
    ok = allowed[row] if 0 <= row < allowed.shape[0] else np.zeros(cap, bool)
    return (dead | ~ok).astype(np.uint8)


def scan_topk(storage, query, codebook, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list, k,
              distance="euclidean", centroids=None, cells=None):
    """(values f32 [nq, k], address i64 [nq, k]); residual codes when `centroids` [n_cells, d] and `cells`
    [nq, max_nprobe] are given; filter_of_query i32 [nq] or None: row 0"""
    nq = query.shape[1]
    rows = np.zeros(nq, np.int64) if filter_of_query is None else np.asarray(filter_of_query, np.int64)
    out_v = np.full((nq, k), -np.inf, np.float32)
    out_a = np.full((nq, k), -1, np.int64)
    for row in np.unique(rows):
        mask = row_mask(is_empty, allowed, int(row))
        if centroids is None:
            v, a = porc.scan_topk(storage, query, codebook, mask, cell_start, cell_size, n_probe_list, k, distance)
        else:
            v, a = rorc.scan_topk(storage, query, codebook, centroids, cells, mask, cell_start, cell_size,
                                  n_probe_list, k, distance)
        out_v[rows == row], out_a[rows == row] = v[rows == row], a[rows == row]
    return out_v, out_a


def search_filtered(query, codebook, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list,
                    id_sets, filter_of_query, k, distance="euclidean", centroids=None):
    """IVFPQ4Index.search_filtered on the index's own state and the cells its coarse step returned (query already
    normalised for "cosine"; centroids [n_cells, d] with pq_use_residual): (values, ids, address).  A filter row
    allows the slots whose id is in the set (an id the index does not hold allows nothing)"""
    allowed = np.stack([(address2id >= 0) & np.isin(address2id, np.asarray(ids, np.int64)) for ids in id_sets])
    v, a = scan_topk(storage, query, codebook, is_empty, allowed, filter_of_query, cell_start[cells],
                     cell_size[cells], n_probe_list, k, "euclidean" if distance == "euclidean" else "inner",
                     centroids=centroids, cells=None if centroids is None else cells)
    return v, np.where(a >= 0, address2id[np.maximum(a, 0)], -1), a
