"""NumPy oracle of IVFPQIndex range search (tpq_ivfpq_range_count / _fill and their residual forms; semantics:
include/torchpq_amd.h), built on the top-k oracle (oracle/ivfpq_oracle.py): its probe walk (probed_slots), its value
(scan_values) and the per-probe arithmetic of its scan_topk_residual.  What this file adds is the storage cut -- only
slots inside [0, capacity) count -- and the threshold.

A hit of query q is a candidate of the top-k scan -- a slot of its first n_probe_list[q] probed cells (clamped to
[0, max_nprobe]; a probe whose start equals the previous probe's start is skipped), inside the storage, not
tombstoned -- whose value is >= threshold[q]; a NaN value or a NaN threshold fails the compare.  Hits come in scan
order: probe rank ascending, then address ascending; a slot of two overlapping cells appears twice.
"""
import numpy as np

from oracle import ivfpq_oracle as orc

F32 = np.float32


def probe_slots(cell_start_q, cell_size_q, n_probe, capacity):
    """one query: per probe rank below the clamped n_probe, the slots scanned for it (empty for a skipped probe), cut
    to the storage.  The walk is orc.probed_slots': the slots of rank p are what the first p + 1 probes add to the
    first p."""
    n = min(max(int(n_probe), 0), len(cell_start_q))
    out, done = [], 0
    for p in range(n):
        upto = orc.probed_slots(cell_start_q, cell_size_q, p + 1)
        s = upto[done:]
        done = len(upto)
        out.append(s[(s >= 0) & (s < capacity)])
    return out


def _live(slots, is_empty):
    return slots if is_empty is None else slots[is_empty[slots] == 0]


def candidates(storage, lut, is_empty, cell_start, cell_size, n_probe_list):
    """plain PQ: per query (slots i64, values f32) of its live candidates, in scan order.
    storage u8 [m/4, capacity, 4], lut f32 [m, nq, 256]"""
    capacity = storage.shape[1]
    out = []
    for q in range(cell_start.shape[0]):
        per_probe = probe_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity)
        s = _live(np.concatenate(per_probe + [np.zeros(0, np.int64)]), is_empty)
        out.append((s, orc.scan_values(storage, lut[:, q, :], s)))
    return out


def candidates_residual(storage, part1, part2, cells, base_sims, is_empty, cell_start, cell_size, n_probe_list,
                        full=None):
    """residual PQ: per query (slots, values); the value of a slot of probe p starts at base_sims[q, p] and adds
    LUT_p[j][code_j] for j ascending, LUT_p = part1[q] + part2[cells[q, p]] (one fp32 add per entry) or full[q, p]
    (orc.scan_topk_residual's arithmetic), and is stored as v + 0.0f"""
    g, capacity, cs4 = storage.shape
    m = g * cs4
    out = []
    for q in range(cell_start.shape[0]):
        all_s, all_v = [np.zeros(0, np.int64)], [np.zeros(0, F32)]
        for p, s in enumerate(probe_slots(cell_start[q], cell_size[q], n_probe_list[q], capacity)):
            s = _live(s, is_empty)
            if s.size == 0:
                continue
            if full is not None:
                lut_p = full[q, p].astype(F32)
            else:
                lut_p = (part1[q].astype(F32) + part2[int(cells[q, p])].astype(F32)).astype(F32)
            v = np.full(s.shape[0], F32(base_sims[q, p]), dtype=F32)
            for j in range(m):
                v = (v + lut_p[j, storage[j // cs4, s, j % cs4]]).astype(F32)
            all_s.append(s)
            all_v.append((v + F32(0.0)).astype(F32))
        out.append((np.concatenate(all_s), np.concatenate(all_v)))
    return out


def hits(cand, threshold):
    """the threshold applied to candidates() / candidates_residual(): (lims i64 [nq + 1], values f32 [total], address
    i64 [total]); `threshold` a float or f32 [nq]; the candidates' values are never changed"""
    nq = len(cand)
    threshold = np.broadcast_to(np.asarray(threshold, F32), (nq,))
    lims, vals, adr = np.zeros(nq + 1, np.int64), [np.zeros(0, F32)], [np.zeros(0, np.int64)]
    for q, (s, v) in enumerate(cand):
        with np.errstate(invalid="ignore"):
            hit = v >= threshold[q]              # False for a NaN on either side
        vals.append(v[hit])
        adr.append(s[hit])
        lims[q + 1] = lims[q] + int(hit.sum())
    return lims, np.concatenate(vals).astype(F32), np.concatenate(adr).astype(np.int64)


def range_scan(storage, lut, is_empty, cell_start, cell_size, n_probe_list, threshold, cand=None):
    """tpq_ivfpq_range_count + _fill.  `cand`: what candidates() returned for the same inputs, when several
    thresholds are applied to them (the values are computed once)"""
    if cand is None:
        cand = candidates(storage, lut, is_empty, cell_start, cell_size, n_probe_list)
    return hits(cand, threshold)


def range_scan_residual(storage, part1, part2, cells, base_sims, is_empty, cell_start, cell_size, n_probe_list,
                        threshold, full=None, cand=None):
    """tpq_ivfpq_range_residual_count + _fill"""
    if cand is None:
        cand = candidates_residual(storage, part1, part2, cells, base_sims, is_empty, cell_start, cell_size,
                                   n_probe_list, full)
    return hits(cand, threshold)


def sort_segments(lims, values, address, *more):
    """each query's segment by (value descending, address ascending): what range_search(sort=True) returns"""
    order = np.concatenate([lo + np.lexsort((address[lo:hi], -values[lo:hi].astype(np.float64)))
                            for lo, hi in zip(lims[:-1], lims[1:])] + [np.zeros(0, np.int64)]).astype(np.int64)
    return tuple(t[order] for t in (values, address, *more))


def range_search(storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list, threshold, lut=None,
                 residual=None):
    """IVFPQIndex.range_search on the index's own state and the cells its coarse step returned: (lims, values, ids,
    address).  Plain PQ: `lut` [m, nq, 256] of the (prepared) queries; residual PQ: `residual` = dict(base_sims=...,
    and part1=, part2= or full=)"""
    cs, sz = cell_start[cells], cell_size[cells]
    if residual is None:
        lims, v, a = range_scan(storage, lut, is_empty, cs, sz, n_probe_list, threshold)
    else:
        lims, v, a = range_scan_residual(storage, residual.get("part1"), residual.get("part2"), cells,
                                         residual["base_sims"], is_empty, cs, sz, n_probe_list, threshold,
                                         full=residual.get("full"))
    return lims, v, address2id[a], a
