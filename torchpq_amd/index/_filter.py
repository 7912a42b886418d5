"""Id filters for filtered search (IVFPQIndex.search_filtered, IVFPQ4Index.search_filtered, IVFFlatIndex.search_filtered /
range_search_filtered): sets of ids kept over the container's slot addresses in the form the index's list scan tests --
rows of bits for IVFPQIndex (csrc/scan_filtered.hip) and IVFPQ4Index (csrc/scan_pq4_filtered.hip), rows of skip bytes
for IVFFlatIndex (the `is_empty` mask of csrc/scan_flat.hip)."""
import torch

from ..kernels import SlotFilterBuildHip


class IdFilter:
    """One or more sets of allowed ids of a container (`index.id_filter(ids)`).

    The object keeps the ids.  Its bit rows -- int32 [n_filters, ceil(capacity / 32) rounded up to a multiple of four
    words], bit a & 31 of word a >> 5 for address a -- are built on first use from the container's id-to-address
    look-up, and built again whenever the container's `_codes_version` has moved: add, remove, growth and compaction
    all move addresses or liveness, so a filter made before an add stays correct after it.  Ids the container does not
    hold are ignored (a later add of such an id makes it count).  `bits()` is what the filtered scans of IVFPQIndex
    and IVFPQ4Index read;
    `masks()` is the same sets as skip masks, uint8 [n_filters, capacity], which IVFFlatIndex hands its list scan and
    its range search in the place of the tombstones -- kept and rebuilt by the same rule."""

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
        self._masks = None
        self._masks_version = None
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

    def masks(self, container=None):
        """the rows as skip masks for the container's present state: uint8 [n_filters, capacity], 0 exactly at the live
        addresses of the row's ids and 1 everywhere else, so the tombstones and the free slots between the cells stay
        skipped whatever the ids say"""
        c = self._container
        assert container is None or container is c, "the filter was made by another index"
        cap = c.capacity
        if self._masks is None or self._masks_version != c._codes_version or self._masks.shape[1] != cap:
            masks = torch.empty(self.n_filters, cap, device=c.device, dtype=torch.uint8)
            dead = c._is_empty != 0
            for row, ids in zip(masks, self.ids):
                allowed = torch.zeros(cap + 1, device=c.device, dtype=torch.bool)
                if ids.numel():
                    address = c.get_address_by_id(ids)
                    inside = (address >= 0) & (address < cap)
                    allowed[torch.where(inside, address, torch.full_like(address, cap))] = True   # (cap: thrown away)
                row.copy_(~allowed[:cap] | dead)
            self._masks, self._masks_version = masks, c._codes_version
        return self._masks


def checked_filter_rows(index, x, flt, filter_of_query):
    """the checks of a filtered search's (flt, filter_of_query) -> the rows as int32 on the index's device, or None"""
    assert isinstance(flt, IdFilter), "flt is what index.id_filter(ids) returns"
    if filter_of_query is not None:
        assert torch.is_tensor(filter_of_query) and filter_of_query.shape == (x.shape[1],)
        assert filter_of_query.dtype in (torch.int32, torch.int64)
        filter_of_query = filter_of_query.to(device=index.device, dtype=torch.int32)
    return filter_of_query


def filtered_search_batches(index, x, flt, filter_of_query, per_batch):
    """search_filtered() of an IVF index: the checks of `filter_of_query`, then the index's batch loop with the rows
    cut alongside the queries; per_batch(xb, rows, sims, cells, n_probe_list, extents)"""
    return index._search_batches(x, per_batch, alongside=(checked_filter_rows(index, x, flt, filter_of_query),))


def queries_by_row(filter_of_query, n_query, n_filters, device):
    """The launches of a scan that takes ONE mask per launch: [(row, queries)], `queries` an int64 tensor of the
    queries that use `row`, ascending -- or None for all of them, in which case nothing is read back.  Queries whose
    row is outside [0, n_filters) are in no group.  With rows given, this reads them back: the one host
    synchronisation of a batch."""
    if filter_of_query is None:
        return [(0, None)]
    rows = filter_of_query.to("cpu", torch.int64)
    assert rows.shape == (n_query,)
    order = torch.argsort(rows, stable=True)
    present, counts = torch.unique_consecutive(rows[order], return_counts=True)
    groups = []
    for row, chunk in zip(present.tolist(), torch.split(order, counts.tolist())):
        if 0 <= row < n_filters:
            groups.append((row, None if chunk.numel() == n_query else chunk.to(device)))
    return groups
