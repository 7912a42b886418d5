"""What the range searches of FlatIndex and IVFFlatIndex share."""
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
