"""NumPy oracle of IVFPQIndex filtered search (tpq_ivfpq_scan_filtered_topk / _residual_topk, tpq_slot_filter_build;
semantics: include/torchpq_amd.h), built on the range oracle (tests/ivfpq_range_oracle.py): its candidates -- the
probe walk, the storage cut, the tombstones, the values -- with `is_empty | ~allowed_row` as the tombstone mask of every
query, then the k best by (value descending, address ascending), NaN removed, padded with (-inf, -1).
"""
import numpy as np

import ivfpq_range_oracle as rorc

F32 = np.float32


def pack_bits(allowed):
    """bool [n_filters, n] -> u32 [n_filters, ceil(n / 32)]: bit s & 31 of word s >> 5"""
    allowed = np.atleast_2d(np.asarray(allowed, bool))
    n_filters, n = allowed.shape
    words = (n + 31) // 32
    padded = np.zeros((n_filters, words * 32), bool)
    padded[:, :n] = allowed
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (padded.reshape(n_filters, words, 32).astype(np.uint64) * weights).sum(-1).astype(np.uint32)


def unpack_bits(bits, n):
    """u32 [n_filters, stride] -> bool [n_filters, n]: the bits of slots >= n are never looked at"""
    bits = np.atleast_2d(np.asarray(bits).view(np.uint32))
    s = np.arange(n)
    return ((bits[:, s >> 5] >> (s & 31).astype(np.uint32)) & 1).astype(bool)


def build_bits(address, n_slots, stride=None):
    """tpq_slot_filter_build on a zeroed row: u32 [stride]; addresses outside [0, n_slots) are ignored"""
    address = np.asarray(address, np.int64)
    allowed = np.zeros(n_slots, bool)
    allowed[address[(address >= 0) & (address < n_slots)]] = True
    row = pack_bits(allowed)[0]
    if stride is not None:
        row = np.concatenate([row, np.zeros(stride - len(row), np.uint32)])
    return row


def query_masks(is_empty, allowed, filter_of_query, nq):
    """per query the tombstone mask `is_empty | ~allowed_row` (u8 [capacity]); a row outside [0, n_filters) allows
    nothing; filter_of_query None: row 0"""
    allowed = np.atleast_2d(np.asarray(allowed, bool))
    cap = allowed.shape[1]
    dead = np.zeros(cap, bool) if is_empty is None else np.asarray(is_empty) != 0
    rows = np.zeros(nq, np.int64) if filter_of_query is None else np.asarray(filter_of_query, np.int64)
    out = []
    for q in range(nq):
        ok = allowed[rows[q]] if 0 <= rows[q] < allowed.shape[0] else np.zeros(cap, bool)
        out.append((dead | ~ok).astype(np.uint8))
    return out


def topk(cand, k):
    """per-query candidates (slots, values) -> (values f32 [nq, k], address i64 [nq, k])"""
    nq = len(cand)
    vals = np.full((nq, k), -np.inf, F32)
    adr = np.full((nq, k), -1, np.int64)
    for q, (s, v) in enumerate(cand):
        keep = ~np.isnan(v)
        s, v = s[keep], v[keep]
        order = np.lexsort((s, -v.astype(np.float64)))[:k]
        vals[q, :len(order)] = v[order]
        adr[q, :len(order)] = s[order]
    return vals, adr


def _per_query(fn, masks):
    """fn(q-slice, mask) for every query with its own mask: the range oracle takes one mask per call"""
    out = []
    for q, mask in enumerate(masks):
        out.extend(fn(slice(q, q + 1), mask))
    return out


def candidates(storage, lut, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list):
    """plain PQ: per query (slots, values) of its allowed live candidates, in scan order"""
    nq = cell_start.shape[0]
    masks = query_masks(is_empty, allowed, filter_of_query, nq)
    return _per_query(lambda q, mask: rorc.candidates(storage, lut[:, q], mask, cell_start[q], cell_size[q],
                                                      n_probe_list[q]), masks)


def candidates_residual(storage, part1, part2, cells, base_sims, is_empty, allowed, filter_of_query, cell_start,
                        cell_size, n_probe_list, full=None):
    nq = cell_start.shape[0]
    masks = query_masks(is_empty, allowed, filter_of_query, nq)
    return _per_query(lambda q, mask: rorc.candidates_residual(
        storage, None if part1 is None else part1[q], part2, cells[q], base_sims[q], mask, cell_start[q],
        cell_size[q], n_probe_list[q], full=None if full is None else full[q]), masks)


def scan_filtered(storage, lut, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list, k):
    """tpq_ivfpq_scan_filtered_topk"""
    return topk(candidates(storage, lut, is_empty, allowed, filter_of_query, cell_start, cell_size, n_probe_list), k)


def scan_filtered_residual(storage, part1, part2, cells, base_sims, is_empty, allowed, filter_of_query, cell_start,
                           cell_size, n_probe_list, k, full=None):
    """tpq_ivfpq_scan_filtered_residual_topk"""
    return topk(candidates_residual(storage, part1, part2, cells, base_sims, is_empty, allowed, filter_of_query,
                                    cell_start, cell_size, n_probe_list, full=full), k)


def search_filtered(storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, id_sets,
                    filter_of_query, k, lut=None, residual=None):
    """IVFPQIndex.search_filtered on the index's own state and the cells its coarse step returned: (values, ids,
    address).  A filter row allows the slots whose id is in the set (an id the index does not hold allows nothing)"""
    allowed = np.stack([(address2id >= 0) & np.isin(address2id, np.asarray(ids, np.int64)) for ids in id_sets])
    cs, sz = cell_start[cells], cell_size[cells]
    if residual is None:
        v, a = scan_filtered(storage, lut, is_empty, allowed, filter_of_query, cs, sz, n_probe_list, k)
    else:
        v, a = scan_filtered_residual(storage, residual.get("part1"), residual.get("part2"), cells,
                                      residual["base_sims"], is_empty, allowed, filter_of_query, cs, sz, n_probe_list,
                                      k, full=residual.get("full"))
    return v, np.where(a >= 0, address2id[np.maximum(a, 0)], -1), a
