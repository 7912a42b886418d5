"""Id filters for filtered search (IVFPQIndex.search_filtered): sets of ids kept as rows of bits over the container's
slot addresses, which is what the list scan tests (csrc/scan_filtered.hip)."""
import torch

from ..kernels import SlotFilterBuildHip


class IdFilter:
    """One or more sets of allowed ids of a container (`index.id_filter(ids)`).

    The object keeps the ids.  Its bit rows -- int32 [n_filters, ceil(capacity / 32) rounded up to a multiple of four
    words], bit a & 31 of word a >> 5 for address a -- are built on first use from the container's id-to-address
    look-up, and built again whenever the container's `_codes_version` has moved: add, remove, growth and compaction
    all move addresses or liveness, so a filter made before an add stays correct after it.  Ids the container does not
    hold are ignored (a later add of such an id makes it count)."""

    def __init__(self, container, ids):
        if torch.is_tensor(ids):
            ids = [ids]
        ids = list(ids)
        assert len(ids) >= 1, "at least one id set"
        for t in ids:
            assert torch.is_tensor(t) and t.dim() == 1 and t.dtype == torch.int64, "an id set is a 1-d int64 tensor"
        self._container = container
        self.ids = [t.to(container.device).contiguous() for t in ids]
        self._bits = None
        self._version = None
        self._build = SlotFilterBuildHip()

    @property
    def n_filters(self):
        return len(self.ids)

    def bits(self, container=None):
        """the rows for the container's present state"""
        c = self._container
        assert container is None or container is c, "the filter was made by another index"
        if self._bits is None or self._version != c._codes_version or self._bits.shape[1] * 32 < c.capacity:
            stride = ((c.capacity + 31) // 32 + 3) // 4 * 4
            bits = torch.zeros(self.n_filters, max(stride, 4), device=c.device, dtype=torch.int32)
            for row, ids in zip(bits, self.ids):
                if ids.numel():
                    self._build(c.get_address_by_id(ids), row, c.capacity)
            self._bits, self._version = bits, c._codes_version
        return self._bits


def filtered_search_batches(index, x, flt, filter_of_query, per_batch):
    """search_filtered() of an IVF index: the checks of `filter_of_query`, then the index's batch loop with the rows
    cut alongside the queries; per_batch(xb, rows, sims, cells, n_probe_list, extents)"""
    assert isinstance(flt, IdFilter), "flt is what index.id_filter(ids) returns"
    if filter_of_query is not None:
        assert torch.is_tensor(filter_of_query) and filter_of_query.shape == (x.shape[1],)
        assert filter_of_query.dtype in (torch.int32, torch.int64)
        filter_of_query = filter_of_query.to(device=index.device, dtype=torch.int32)
    return index._search_batches(x, per_batch, alongside=(filter_of_query,))
