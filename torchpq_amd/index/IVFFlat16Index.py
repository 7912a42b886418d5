"""IVFFlat16Index: IVFFlatIndex with the vectors stored as fp16 -- half the memory and half the list traffic, nothing
trained.

The container is CellContainer unchanged.  A vector of d components is rows = ceil(d / 2) 32-bit words: word r holds
component 2r as an IEEE half in its low 16 bits and component 2r + 1 in its high 16 bits (for odd d the last high half
is +0 and is never read into a value).  code_size = 4 rows and contiguous_size = 4, so `_storage` is uint8
[rows, capacity, 4] and `_storage.view(torch.int32)` is [rows, capacity, 1]: row-major over dimension pairs and
slot-contiguous, which the list scan (tpq_ivf_flat16_scan_topk, csrc/scan_flat_f16.hip) reads in place.  add / expand /
remove / tombstones / `_address2id` / state_dict and the IdFilter masks work on code bytes as they do for IVFFlatIndex.

Values are those of IVFFlatIndex over the rounded vectors, bit for bit: every result equals what an IVFFlatIndex with
the same coarse codebook returns after add(x.half().float()) (include/torchpq_amd.h).

`use_cell_major` (off by default) works as on IVFFlatIndex: a batch of at least `cell_major_min_batch` queries with
k <= 256 and more probes than the route's `first_probe` takes the cell-major scan (tpq_ivf_flat16_cells_topk,
csrc/scan_flat_f16_cells.hip), which feeds the stored halves to the fp16 matrix cores as they lie and returns the same
values, ids and addresses bit for bit.  The fp16 tile takes whole groups of 8 dimensions: with a `d_vector` that is not
a multiple of 8 the switch changes nothing.  `last_route` is "cell_major" or "query_major", the last search's route.
"""
import torch

from ..container import CellContainer
from ..kernels import IVFFlat16CellTopkHip, IVFFlat16RangeHip, IVFFlat16TopkHip
from .IVFFlatIndex import IVFFlatIndex


class IVFFlat16Index(IVFFlatIndex):
    def __init__(self, d_vector, n_cells=128, initial_size=None, expand_step_size=128, expand_mode="double",
                 distance="euclidean", device="cuda:0", verbose=0):
        assert d_vector >= 1
        assert distance in ("euclidean", "cosine")
        if torch.device(device).type == "cuda":
            assert torch.cuda.is_available(), "cuda is not available"
        # (the container's constructor, not IVFFlatIndex's: the code size is this layout's)
        CellContainer.__init__(self, code_size=4 * ((d_vector + 1) // 2), n_cells=n_cells, dtype="uint8",
                               device=device, initial_size=initial_size, expand_step_size=expand_step_size,
                               expand_mode=expand_mode, use_inverse_id_mapping=True, contiguous_size=4,
                               verbose=verbose)
        self.d_vector = d_vector
        self.distance = distance
        self.verbose = verbose
        self.use_cublas = True
        self._init_coarse(n_cells, verbose)
        self._flat_topk = IVFFlat16TopkHip()
        self._flat_range = IVFFlat16RangeHip()
        self._flat_cells = IVFFlat16CellTopkHip()   # the cell-major route (the module's docstring); off by default
        self.use_cell_major = False
        self.cell_major_min_batch = 1024
        self.last_route = None
        self.to(device)

    # ---- the byte layout -----------------------------------------------------------------------------
    @staticmethod
    def vectors_to_codes(x):
        """[d, n] float32 -> the container's code rows [4 ceil(d / 2), n] uint8, rounded to nearest even: rows 4 r and
        4 r + 1 are the bytes of half(x[2 r]), rows 4 r + 2 and 4 r + 3 those of half(x[2 r + 1]) (+0 beyond an odd d)"""
        d, n = x.shape
        rows = (d + 1) // 2
        h = torch.zeros(2 * rows, n, dtype=torch.float16, device=x.device)
        h[:d] = x.to(torch.float16)
        return h.view(torch.uint8).reshape(rows, 2, n, 2).permute(0, 1, 3, 2).reshape(4 * rows, n)

    @staticmethod
    def codes_to_vectors(codes, d=None):
        """[4 rows, n] uint8 -> [d, n] float32 of the stored halves (d = 2 rows when not given: an odd d's pad
        included); the inverse of vectors_to_codes on values fp16 holds"""
        r4, n = codes.shape
        h = codes.reshape(r4 // 4, 2, 2, n).permute(0, 1, 3, 2).contiguous().view(torch.float16)
        return h.reshape(r4 // 2, n)[:d].float()

    def _vectors(self):
        """the stored vectors as the scan reads them, [ceil(d_vector / 2), capacity] int32 (a view of `_storage`)"""
        return self._storage.view(torch.int32)[:, :, 0]

    # ---- add / reconstruct -----------------------------------------------------------------------------
    def add(self, x, ids=None, return_address=False):
        """x [d_vector, n] f32 (normalised in fp32 for "cosine"), then rounded to nearest even with .to(float16) and
        stored; the cell is that of the rounded vector.  Optional ids [n] int64 (default arange + max_id + 1);
        returns ids (and the slot addresses if return_address)."""
        assert x.dtype == torch.float32
        x = self._prepare(x)
        assert self.vq_codec.is_trained, "index is not trained"
        assigned_cells = self.vq_codec.encode(x.to(torch.float16).float())
        return CellContainer.add(self, self.vectors_to_codes(x), cells=assigned_cells, ids=ids,
                                 return_address=return_address)

    def reconstruct(self, ids=None, address=None):
        """the stored vectors [d_vector, n] f32 of `ids` (or of slot addresses): the fp32 of the stored halves; zero
        columns for unknown ids / invalid addresses"""
        return super().reconstruct(ids=ids, address=address)[:self.d_vector]

    # ---- search ----------------------------------------------------------------------------------------
    # (search_cells is IVFFlatIndex's: `_flat_topk`, `_flat_cells` and `_vectors()` are this storage's)
    def _cell_major_serves_d(self):
        """the fp16 tile takes whole k-groups of 8 dimensions: any other d_vector keeps the query-major scan"""
        return self.d_vector % 8 == 0
