"""What the range searches of FlatIndex, IVFFlatIndex, IVFPQIndex and IVFPQ4Index share."""
import torch


def sort_range_hits(lims, vals, ids, address):
    """range_search(sort=True): each query's segment [lims[q], lims[q+1]) ordered by value descending, equal values
    by address ascending -> (vals, ids, address)"""
    total = vals.numel()
    if not total:
        return vals, ids, address
    # three stable sorts, least significant key first: address, value (descending), query
    order = torch.argsort(address, stable=True)
    order = order[torch.argsort(vals[order], descending=True, stable=True)]
    query_of = torch.repeat_interleave(torch.arange(lims.numel() - 1, device=lims.device), lims.diff(),
                                       output_size=total)
    order = order[torch.argsort(query_of[order], stable=True)]
    return vals[order], ids[order], address[order]


def range_search_batches(index, x, threshold, per_batch, return_address, sort, alongside=()):
    """range_search() of an IVF index (a CoarseProbeMixin) over batches of `max_query_batch` prepared queries: the
    coarse step per batch, then per_batch(xb, thr, sims, cells, n_probe_list, extents) -- the index's
    range_search_cells -- which returns (lims, values, ids, address); a later batch's lims offset by the hits of the
    earlier ones, the concatenation (or the empty result), the sort -> (lims, values, ids[, address]).
    `alongside`: per-query tensors [n_query, ...] (or None), cut as the queries are and handed to per_batch behind thr
    (CoarseProbeMixin._search_batches does the same)"""
    n_query = x.shape[1]
    if torch.is_tensor(threshold):
        assert threshold.shape == (n_query,) and threshold.dtype == torch.float32
        threshold = threshold.to(index.device)
    lims = [torch.zeros(1, device=index.device, dtype=torch.int64)]
    vals, ids, address, total = [], [], [], 0
    for q0 in range(0, n_query, index.max_query_batch):
        xb = x[:, q0:q0 + index.max_query_batch].contiguous()
        thr = threshold[q0:q0 + index.max_query_batch] if torch.is_tensor(threshold) else threshold
        cut = tuple(None if t is None else t[q0:q0 + index.max_query_batch].contiguous() for t in alongside)
        lb, vb, ib, ab = per_batch(xb, thr, *cut, *index._probe_with_extents(xb))
        lims.append(lb[1:] + total)          # a later batch's segments start where the earlier ones end
        vals.append(vb)
        ids.append(ib)
        address.append(ab)
        total += vb.numel()
    lims = torch.cat(lims)
    if vals:
        vals, ids, address = torch.cat(vals), torch.cat(ids), torch.cat(address)
    else:
        vals = torch.empty(0, device=index.device, dtype=torch.float32)
        ids = address = torch.empty(0, device=index.device, dtype=torch.int64)
    if sort:
        vals, ids, address = sort_range_hits(lims, vals, ids, address)
    return (lims, vals, ids, address) if return_address else (lims, vals, ids)
