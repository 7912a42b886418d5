"""Exact (brute-force) search: drop-in for torchpq.index.FlatIndex (reference index/FlatIndex.py:8-101
over container/FlatContainer.py).  SURVEY 8(f) rank 4: the ground-truth generator for recall.

search = one library GEMM (rocBLAS, as the reference uses cuBLAS) + the HIP row top-k select
(tpq_topk_select) + address->id; with `use_fused_search = True` one fused HIP similarity + top-k
(tpq_flat_topk) that never forms the [n_query, capacity] matrix.  range_search = the same HIP similarity tiles with a
count and a fill pass (tpq_flat_range_count / tpq_flat_range_fill).  Storage is the reference's dense `_storage [d, capacity, 1]`
with `_address2id`; vectors are appended, removed slots are tombstoned (id -1) and reused.
"""
import torch

from .. import metric, util
from ..container.BaseContainer import BaseContainer
from ..fn import Topk
from ..kernels import FlatRangeHip, FlatTopkHip
from ._range import sort_range_hits


class FlatIndex(BaseContainer):
    # Opt-in route of search(): tpq_flat_topk on _storage and _address2id, O(n_query k) temporary memory at any
    # capacity, queries in batches of max_query_batch.  It ranks by the same similarity as the default route for every
    # distance ("cosine": queries AND stored vectors divided by their norms, the latter in a [d, capacity] temporary per
    # call); the values are the fp32-MFMA chains of include/torchpq_amd.h where the default route's are the library
    # GEMM's, so low bits differ.  The kernel's limit is min(k, capacity) <= 1024: beyond it search() raises ValueError
    # (the default route has no such limit).  Plain attributes, not constructor arguments (the signature is the
    # reference's) and not part of the state_dict.
    use_fused_search = False
    max_query_batch = 32768

    def __init__(self, d_vector, initial_size=None, expand_step_size=1024, expand_mode="double",
                 device="cuda:0", distance="euclidean", verbose=0):
        super().__init__(device=device, initial_size=initial_size, expand_step_size=expand_step_size,
                         expand_mode=expand_mode, use_inverse_id_mapping=True)
        self.d_vector = d_vector
        self.code_size = d_vector
        self.contiguous_size = 1
        self.dtype = torch.float32
        self.verbose = verbose
        if distance in ["euclidean", "l2"]:
            self.distance = "euclidean"
        elif distance in ["cosine", "angular"]:
            self.distance = "cosine"
        elif distance in ["inner", "dot"]:
            self.distance = "inner"
        elif distance in ["manhattan", "l1"]:
            raise NotImplementedError("currently manhattan distance is not supported")
        else:
            raise NotImplementedError(f"unknown distance metric: {distance}")
        self._n_items = 0
        self.register_buffer("_storage", torch.zeros(d_vector, self.initial_size, 1, device=device,
                                                     dtype=torch.float32))
        self._topk = Topk()
        self._flat_topk = FlatTopkHip()
        self._flat_range = FlatRangeHip()

    @property
    def n_items(self):
        return self._n_items

    def _after_load_state_dict(self):
        super()._after_load_state_dict()
        self._n_items = int((self._address2id >= 0).sum().item())

    def _grow_to(self, needed):
        cap = self.capacity
        if needed <= cap:
            return
        new_cap = cap
        step = self.expand_step_size
        while new_cap < needed:
            new_cap = max(new_cap * 2, 1) if self.expand_mode == "double" else new_cap + step
        storage = torch.zeros(self.d_vector, new_cap, 1, device=self.device, dtype=torch.float32)
        storage[:, :cap] = self._storage
        a2i = torch.full((new_cap,), -1, device=self.device, dtype=torch.long)
        a2i[:cap] = self._address2id
        del self._storage, self._address2id
        self.register_buffer("_storage", storage)
        self.register_buffer("_address2id", a2i)

    def add(self, x, ids=None, return_address=False):
        """x [d_vector, n] f32; ids default arange + max_id + 1; free slots are filled in order."""
        assert len(x.shape) == 2 and x.shape[0] == self.d_vector
        assert util.check_dtype(x, "float32")
        x = x.to(self.device)
        n = x.shape[1]
        if ids is None:
            ids = torch.arange(n, device=self.device, dtype=torch.long) + self.max_id + 1
        else:
            assert util.check_dtype(ids, torch.int64) and ids.shape[0] == n
            ids = ids.to(self.device)
        if n == 0:
            return (ids, ids.clone()) if return_address else ids
        self._grow_to(self._n_items + n)
        free = torch.nonzero(self._address2id < 0)[:n, 0]
        self._storage[:, free, 0] = x
        self._address2id[free] = ids
        self._max_id = max(self._max_id, ids.max().item())
        self._n_items += n
        self._drop_inverse_id_mapping()
        return (ids, free) if return_address else ids

    def remove(self, ids=None, address=None):
        if ids is not None:
            address = self.get_address_by_id(ids)
        elif address is None:
            raise RuntimeError("Need either ids or address")
        address = address.to(self.device)
        address = address[(address >= 0) & (address < self.capacity)].unique()
        address = address[self._address2id[address] >= 0]
        if address.shape[0] == 0:
            return
        self._address2id[address] = -1
        self._storage[:, address] = 0
        self._n_items -= address.shape[0]
        self._drop_inverse_id_mapping()

    def search(self, x, k=1, return_address=False):
        """x [d_vector, n_query] f32 -> (values [n_query, k] descending, ids[, address])"""
        d_vector, n_query = x.shape
        assert d_vector == self.d_vector
        assert util.check_dtype(x, "float32")
        assert k >= 1
        x = x.to(self.device)
        if self.use_fused_search:
            return self._search_fused(x, k, return_address)
        storage = self._storage.view(self.d_vector, -1)
        if self.distance == "euclidean":
            sims = metric.negative_squared_l2_distance(x, storage)
        elif self.distance == "cosine":
            sims = metric.cosine_similarity(x, storage, normalize=True)
        else:
            sims = metric.cosine_similarity(x, storage, normalize=False)
        sims = sims.masked_fill((self._address2id < 0)[None, :], float("-inf")).contiguous()
        topk_val, topk_address = self._topk(sims, k=min(k, sims.shape[1]), dim=1)
        topk_address = torch.where(torch.isneginf(topk_val), torch.full_like(topk_address, -1), topk_address)
        topk_ids = self.get_id_by_address(topk_address)
        if return_address:
            return topk_val, topk_ids, topk_address
        return topk_val, topk_ids

    def _fused_vectors(self):
        """what the fused kernel reads: _storage as it is, or for "cosine" a copy with every stored vector divided by
        (its norm + 1e-8) -- metric.cosine_similarity's normalisation; [d, capacity], never n_query x capacity"""
        if self.distance != "cosine":
            return self._storage
        storage = self._storage.view(self.d_vector, -1)
        return (storage / (storage.norm(dim=-2, keepdim=True) + 1e-8)).contiguous()

    def _search_fused(self, x, k, return_address):
        """search() through tpq_flat_topk: the same conventions -- "cosine" divides queries and stored vectors by
        (norm + 1e-8) as metric.cosine_similarity does, width min(k, capacity), pads (-inf, -1), ids gathered by the
        same call"""
        k = min(k, self.capacity)
        if k > 1024:
            raise ValueError(f"FlatIndex.use_fused_search: min(k, capacity) = {k} is beyond the fused kernel's limit "
                             "of 1024; set use_fused_search = False for this call")
        storage = self._fused_vectors()
        if self.distance == "cosine":
            x = x / (x.norm(dim=-2, keepdim=True) + 1e-8)
        x = x.contiguous()
        parts = [self._flat_topk(storage, x[:, b:b + self.max_query_batch].contiguous(), k,
                                 address2id=self._address2id, distance=self.distance)
                 for b in range(0, max(x.shape[1], 1), self.max_query_batch)]
        topk_val, topk_address, topk_ids = parts[0] if len(parts) == 1 else (torch.cat(t, dim=0) for t in zip(*parts))
        if return_address:
            return topk_val, topk_ids, topk_address
        return topk_val, topk_ids

    def range_search(self, x, threshold, return_address=False, sort=False):
        """x [d_vector, n_query] f32, threshold a float or f32 [n_query] -> (lims int64 [n_query + 1], values f32
        [total], ids int64 [total][, address]): the hits of query q are values[lims[q]:lims[q+1]] and
        ids[lims[q]:lims[q+1]] -- every stored vector whose value is >= threshold, exactly: the whole database is
        walked.  `threshold` is in the index's value space, the one search returns: -squared-L2 for "euclidean" (all
        vectors within distance r: threshold = -r * r), the cosine similarity for "cosine".  Hits come in address
        order; sort=True orders each query's hits by value descending, equal values by address ascending.  Always the
        HIP route (tpq_flat_range_count / tpq_flat_range_fill; values as use_fused_search's), O(n_query) temporary
        memory beside the hits.  Synchronises once per batch of `max_query_batch` queries: the number of hits sizes
        the outputs."""
        d_vector, n_query = x.shape
        assert d_vector == self.d_vector
        assert util.check_dtype(x, "float32")
        x = x.to(self.device)
        if torch.is_tensor(threshold):
            assert threshold.shape == (n_query,) and threshold.dtype == torch.float32
            threshold = threshold.to(self.device)
        storage = self._fused_vectors()
        if self.distance == "cosine":
            x = x / (x.norm(dim=-2, keepdim=True) + 1e-8)
        lims = [torch.zeros(1, device=self.device, dtype=torch.int64)]
        vals, ids, address, total = [], [], [], 0
        for q0 in range(0, n_query, self.max_query_batch):
            thr = threshold[q0:q0 + self.max_query_batch] if torch.is_tensor(threshold) else threshold
            lb, vb, ab, ib = self._flat_range(storage, x[:, q0:q0 + self.max_query_batch].contiguous(), thr,
                                              address2id=self._address2id, distance=self.distance)
            lims.append(lb[1:] + total)          # a later batch's segments start where the earlier ones end
            vals.append(vb)
            ids.append(ib)
            address.append(ab)
            total += vb.numel()
        lims = torch.cat(lims)
        if vals:
            vals, ids, address = torch.cat(vals), torch.cat(ids), torch.cat(address)
        else:
            vals = torch.empty(0, device=self.device, dtype=torch.float32)
            ids, address = (torch.empty(0, device=self.device, dtype=torch.int64) for _ in range(2))
        if sort:
            vals, ids, address = sort_range_hits(lims, vals, ids, address)
        return (lims, vals, ids, address) if return_address else (lims, vals, ids)
