"""The container's kernels: address / id look-ups, cell growth, code decode / scatter / scan-layout packing."""
import torch

from .._lib import load, ptr, require_gpu
from ._common import call
from .scan import packed_chunk_width


class GetIOAHip:
    """Index of appearance (kernels/GetIOACuda.py:36-63): ioa[i] = #{j < i: labels[j] == labels[i]}."""

    def __init__(self, tpb=256):
        pass

    def __call__(self, labels, unique_labels=None, n_cells=None):
        assert labels.dtype == torch.int64 and len(labels.shape) == 1
        labels = labels.contiguous()
        require_gpu(labels)
        n = labels.shape[0]
        ioa = torch.empty_like(labels)
        if n == 0:
            return ioa
        if n_cells is None:
            n_cells = 2 ** 31 - 2  # sort on all 31 key bits
        ws_bytes = load().tpq_get_ioa_workspace_bytes(n)
        ws = torch.empty(ws_bytes, device=labels.device, dtype=torch.uint8)
        call("tpq_get_ioa", labels.device, ptr(labels), ptr(ioa), n, int(n_cells), ptr(ws), ws_bytes)
        return ioa


class GetWriteAddressHip:
    """The ioa-th empty slot of each label's cell (kernels/GetWriteAddressV2Cuda.py:36-66)."""

    def __init__(self, tpb=256):
        pass

    def __call__(self, is_empty, div_start, div_size, labels, ioa):
        assert div_start.shape == div_size.shape
        assert ioa.shape == labels.shape
        require_gpu(is_empty, div_start, div_size, labels, ioa)
        n_slots = is_empty.shape[0]
        n_labels = labels.shape[0]
        out = torch.empty_like(labels)
        call("tpq_get_write_address", labels.device, ptr(is_empty), ptr(div_start), ptr(div_size), ptr(labels),
             ptr(ioa), ptr(out), n_slots, n_labels)
        return out


class GetCellByAddressHip:
    """address -> cell (kernels/GetDivByAddressV2Cuda.py:38-67); ``div_end`` = start + capacity."""

    def __init__(self, ta=4, tpb=256):
        pass

    def __call__(self, address, div_start, div_end):
        assert div_start.shape[0] == div_end.shape[0]
        address = address.contiguous()
        cap = (div_end - div_start).contiguous()
        div_start = div_start.contiguous()
        require_gpu(address, div_start, cap)
        out = torch.empty_like(address)
        call("tpq_get_cell_by_address", address.device, ptr(address), ptr(div_start), ptr(cap), ptr(out),
             address.shape[0], div_start.shape[0])
        return out


class GetIdByAddressHip:
    """address -> id gather with -1 for invalid addresses (container/BaseContainer.py:58-65)."""

    def __call__(self, address2id, address):
        shape = address.shape
        flat = address.contiguous().view(-1)
        require_gpu(address2id, flat)
        out = torch.empty_like(flat)
        call("tpq_get_id_by_address", flat.device, ptr(address2id), address2id.shape[0], ptr(flat), ptr(out),
             flat.shape[0])
        return out.view(shape)


class GetAddressByIdHip:
    """id -> address by comparing every id with every stored id (kernels/GetAddressByIdCuda.py,
    kernels/cuda/get_address_by_id.cu:8-44): the use_inverse_id_mapping=False path of
    BaseContainer.get_address_by_id; smallest matching address, -1 when absent."""

    def __init__(self, tpb=256):
        pass

    def __call__(self, address2id, ids):
        assert address2id.dtype == ids.dtype == torch.int64
        ids = ids.contiguous()
        require_gpu(address2id, ids)
        out = torch.empty_like(ids)
        call("tpq_get_address_by_id", ids.device, ptr(address2id), address2id.shape[0], ptr(ids), ptr(out),
             ids.shape[0])
        return out


class GrowCellsHip:
    """CellContainer.expand in one pass (container/CellContainer.py:249-311): every cell moves to
    its place in the larger layout, new tails initialised free.  Returns the three new buffers."""

    def __call__(self, storage, address2id, is_empty, old_start, old_capacity, new_start, new_capacity,
                 new_slots, out=None):
        """out = (storage, address2id, is_empty) buffers of the new size to fill (must not alias the
        inputs), or None to allocate them"""
        g, old_slots, cs = storage.shape
        assert cs == 4 and storage.dtype == torch.uint8
        require_gpu(storage, address2id, is_empty, old_start, old_capacity, new_start, new_capacity)
        dev = storage.device
        if out is None:
            new_storage = torch.empty(g, new_slots, 4, device=dev, dtype=torch.uint8)
            new_a2i = torch.empty(new_slots, device=dev, dtype=torch.int64)
            new_empty = torch.empty(new_slots, device=dev, dtype=torch.uint8)
        else:
            new_storage, new_a2i, new_empty = out
            assert new_storage.shape == (g, new_slots, 4) and new_storage.is_contiguous()
            assert new_a2i.shape == (new_slots,) and new_empty.shape == (new_slots,)
            assert new_storage.dtype == torch.uint8 and new_a2i.dtype == torch.int64 and new_empty.dtype == torch.uint8
            assert new_storage.data_ptr() != storage.data_ptr() and new_a2i.data_ptr() != address2id.data_ptr()
        call("tpq_grow_cells", dev, ptr(storage), ptr(address2id), ptr(is_empty), ptr(old_start), ptr(old_capacity),
             ptr(new_start), ptr(new_capacity), ptr(new_storage), ptr(new_a2i), ptr(new_empty), old_slots,
             new_slots, old_start.shape[0], g * 4)
        return new_storage, new_a2i, new_empty


class PQDecodeHip:
    """codes -> reconstruction (kernels/PQDecodeCuda.py:43-65)."""

    def __init__(self, tm=2, td=8):
        pass

    def __call__(self, codebook, code):
        m, d, k = codebook.shape
        assert code.shape[0] == m and k == 256
        assert code.dtype == torch.uint8
        codebook = codebook.contiguous()
        code = code.contiguous()
        require_gpu(codebook, code)
        n = code.shape[1]
        out = torch.empty(m * d, n, device=codebook.device, dtype=torch.float32)
        call("tpq_pq_decode", codebook.device, ptr(codebook), ptr(code), ptr(out), m, d, n)
        return out


class ScatterCodesHip:
    """codes [m, n] -> _storage [m/4, cap, 4] (and the scan-layout copy) at `address`
    (CellContainer.set_data_by_address, container/CellContainer.py:213-239)."""

    def __call__(self, codes, address, storage, packed=None):
        m, n = codes.shape
        assert storage.shape[0] * storage.shape[2] == m and storage.shape[2] == 4
        assert address.shape[0] == n and address.dtype == torch.int64
        codes = codes.contiguous()
        address = address.contiguous()
        require_gpu(codes, address, storage, packed)
        call("tpq_scatter_codes", codes.device, ptr(codes), ptr(address), ptr(storage), ptr(packed), m, n,
             storage.shape[1])


class PackCodesHip:
    """(Re)build the MI355X scan layout from _storage for slots [begin, end)."""

    def __call__(self, storage, packed=None, begin=0, end=None):
        g, cap, cs = storage.shape
        assert cs == 4 and storage.dtype == torch.uint8
        m = g * cs
        w = packed_chunk_width(m)
        if packed is None:
            packed = torch.empty(m // w, cap, w, device=storage.device, dtype=torch.uint8)
        assert packed.shape == (m // w, cap, w)
        require_gpu(storage, packed)
        end = cap if end is None else end
        call("tpq_ivfpq_pack_codes", storage.device, ptr(storage), ptr(packed), cap, m, begin, end)
        return packed
