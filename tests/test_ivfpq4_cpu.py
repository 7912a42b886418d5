"""CPU: the 4-bit codes of IVFPQ4Index -- nibble packing, the oracle's reading of the storage, its table and values
against float64, its order, candidates and padding (tests/ivfpq4_oracle.py restates include/torchpq_amd.h), and the
two C entry points' argument checks, which run before any HIP call."""
import numpy as np
import pytest
import torch

import ivfpq4_cases as cases
import ivfpq4_oracle as porc


def test_pack_and_unpack_nibbles_round_trip():
    from torchpq_amd.codec import PQ4Codec
    rng = np.random.default_rng(0)
    labels = rng.integers(0, 16, (24, 37)).astype(np.int64)
    packed = PQ4Codec.pack_nibbles(torch.from_numpy(labels))
    assert packed.dtype == torch.uint8 and packed.shape == (12, 37)
    # an independent expression: byte b = sub-quantizer 2 b + 16 x sub-quantizer 2 b + 1
    want = (labels.reshape(12, 2, 37)[:, 0] + 16 * labels.reshape(12, 2, 37)[:, 1]).astype(np.uint8)
    assert np.array_equal(packed.numpy(), want)
    assert np.array_equal(porc.pack(labels), want)
    back = PQ4Codec.unpack_nibbles(packed)
    assert back.dtype == torch.uint8 and np.array_equal(back.numpy(), labels)
    every = torch.arange(256, dtype=torch.uint8).reshape(1, 256)
    assert torch.equal(PQ4Codec.pack_nibbles(PQ4Codec.unpack_nibbles(every)), every)


def test_oracle_reads_the_storage_as_the_header_says():
    """m = 8, two slots, every nibble of a slot distinct: catches swapped nibbles, byte order and word order"""
    # slot 0: sub-quantizer j holds j; slot 1: sub-quantizer j holds 15 - j
    storage = np.zeros((1, 2, 4), np.uint8)
    storage[0, 0] = [0x10, 0x32, 0x54, 0x76]
    storage[0, 1] = [0xef, 0xcd, 0xab, 0x89]
    codes = porc.unpack(storage)
    assert codes.shape == (8, 2) and codes.dtype == np.uint8
    assert codes[:, 0].tolist() == list(range(8)) and codes[:, 1].tolist() == [15 - j for j in range(8)]
    # the same through the 32-bit word the kernel loads: nibble n of word w is sub-quantizer 8 w + n
    words = storage.view("<u4")[:, :, 0]
    assert [int(words[0, 0] >> (4 * n)) & 15 for n in range(8)] == list(range(8))
    # m = 16: the second word row holds sub-quantizers 8 ... 15, and the container's rows are the packed bytes
    labels = np.stack([np.arange(16), 15 - np.arange(16)], axis=1).astype(np.uint8)     # [m, 2 slots]
    rows = porc.pack(labels)                                                             # [8, 2]
    storage = np.ascontiguousarray(rows.reshape(2, 4, 2).transpose(0, 2, 1))             # [m / 8, slots, 4]
    assert np.array_equal(porc.unpack(storage), labels)
    words = storage.view("<u4")[:, :, 0]
    assert [int(words[1, 0] >> (4 * n)) & 15 for n in range(8)] == list(range(8, 16))


@pytest.mark.parametrize("distance", ["euclidean", "inner"])
@pytest.mark.parametrize("m,ds", [(8, 5), (64, 2), (256, 1)])
def test_oracle_table_and_values_against_float64(m, ds, distance):
    """Every fp32 operation rounds by at most u = 2^-24 relative.  One step of a table entry forms its term with a
    relative error of at most 3 u (difference, square; or one product) and adds it to a running sum no larger than M,
    the sum of the terms' magnitudes: an entry is within (3 + ds) u M of float64 to first order, and 6 ds u M is used.
    A value adds m entries, every partial sum no larger than S = the sum of the entries' M: within (3 + ds + m) u S to
    first order, and 2 (3 ds + m) u S is used."""
    rng = np.random.default_rng(m + ds)
    nq, cap = 7, 50
    cb = rng.standard_normal((m, ds, 16)).astype(np.float32)
    query = rng.standard_normal((m * ds, nq)).astype(np.float32)
    codes = rng.integers(0, 16, (m, cap)).astype(np.uint8)
    table = porc.lut(query, cb, distance)
    assert table.shape == (nq, m, 16) and table.dtype == np.float32
    q64 = query.astype(np.float64).reshape(m, ds, nq).transpose(2, 0, 1)[:, :, :, None]   # [nq, m, ds, 1]
    c64 = cb.astype(np.float64)[None]                                                     # [1, m, ds, 16]
    terms = -(q64 - c64) ** 2 if distance == "euclidean" else q64 * c64
    t64 = terms.sum(2)
    mag = np.abs(terms).sum(2)
    assert np.all(np.abs(table - t64) <= 2 * 3 * ds * 2.0 ** -24 * mag)
    slots = np.arange(cap)
    v = porc.values(table, codes, slots)
    assert v.shape == (nq, cap) and v.dtype == np.float32
    j = np.arange(m)[:, None]
    v64 = np.stack([t64[q][j, codes].sum(0) for q in range(nq)])
    s64 = np.stack([mag[q][j, codes].sum(0) for q in range(nq)])
    assert np.all(np.abs(v - v64) <= 2 * (3 * ds + m) * 2.0 ** -24 * s64)
    assert np.abs(v - v64).max() > 0          # (float32 was used: the comparison is not vacuous)


def _tiny(codes):
    """m = 8, ds = 1 storage from codes [8, cap]; codebook[j][0][c] = c for j == 0, else 0"""
    cap = codes.shape[1]
    rows = porc.pack(codes)
    storage = np.ascontiguousarray(rows.reshape(1, 4, cap).transpose(0, 2, 1))
    cb = np.zeros((8, 1, 16), np.float32)
    cb[0, 0] = np.arange(16)
    return storage, cb


def test_oracle_order_on_ties_padding_and_duplicate_probe():
    codes = np.zeros((8, 12), np.uint8)
    codes[0] = [3, 7, 3, 7, 1, 7, 3, 0, 9, 9, 9, 9]
    storage, cb = _tiny(codes)
    query = np.ones((8, 1), np.float32)                       # inner product: the value of a slot is codes[0]
    cs, sz = np.array([[0, 4]], np.int64), np.array([[4, 4]], np.int64)
    v, a = porc.scan_topk(storage, query, cb, None, cs, sz, np.array([2]), 6, "inner")
    assert a.tolist() == [[1, 3, 5, 0, 2, 6]] and v.tolist() == [[7, 7, 7, 3, 3, 3]]     # equal values: by address
    # padding beyond the candidates
    v, a = porc.scan_topk(storage, query, cb, None, cs, sz, np.array([1]), 6, "inner")
    assert a.tolist() == [[1, 3, 0, 2, -1, -1]] and np.all(np.isneginf(v[0, 4:]))
    # tombstones
    empty = np.zeros(12, np.uint8)
    empty[[1, 5]] = 1
    v, a = porc.scan_topk(storage, query, cb, empty, cs, sz, np.array([2]), 3, "inner")
    assert a.tolist() == [[3, 0, 2]]
    # a probe whose start equals the previous probe's start is skipped, whatever its size; n_probe_list is clamped
    cs2, sz2 = np.array([[0, 0, 8]], np.int64), np.array([[2, 8, 4]], np.int64)
    v, a = porc.scan_topk(storage, query, cb, None, cs2, sz2, np.array([99]), 8, "inner")
    assert a.tolist() == [[8, 9, 10, 11, 1, 0, -1, -1]]
    v, a = porc.scan_topk(storage, query, cb, None, cs2, sz2, np.array([-3]), 2, "inner")
    assert a.tolist() == [[-1, -1]]
    # a cell that leaves the storage is cut
    v, a = porc.scan_topk(storage, query, cb, None, np.array([[10]], np.int64), np.array([[50]], np.int64),
                          np.array([1]), 4, "inner")
    assert a.tolist() == [[10, 11, -1, -1]]


def test_oracle_leaves_nan_values_out():
    codes = np.zeros((8, 6), np.uint8)
    codes[0] = [1, 2, 3, 4, 5, 6]
    storage, cb = _tiny(codes)
    cb[0, 0, 3] = np.nan
    cb[0, 0, 5] = -np.inf
    query = np.ones((8, 1), np.float32)
    v, a = porc.scan_topk(storage, query, cb, None, np.array([[0]], np.int64), np.array([[6]], np.int64),
                          np.array([1]), 6, "inner")
    assert a.tolist() == [[5, 3, 1, 0, 4, -1]]       # -inf keeps its address, NaN never enters
    assert np.isneginf(v[0, 4]) and np.isneginf(v[0, 5]) and not np.isnan(v).any()


def test_summation_order_decides_places_in_the_offset_case():
    """the premise of test_gpu_ivfpq4.test_scan_when_the_summation_order_decides: on those very inputs a pairwise fp32
    sum picks another top-k set than the specification's chain for at least one query"""
    c, k = cases.offset_case()
    table = porc.lut(c["query"], c["codebook"], "inner")
    assert np.array_equal(table, np.broadcast_to(c["codebook"][:, 0, :], table.shape))    # entries = codebook, exactly
    assert np.all(np.abs(table + 2.0 ** 20) < 8)
    _, ea = porc.scan_topk(c["storage"], c["query"], c["codebook"], c["is_empty"], c["cs"], c["sz"], c["npl"], k,
                           "inner")
    pairwise = cases.pairwise_topk_sets(c, k, "inner")
    differ = [q for q in range(len(pairwise)) if pairwise[q] != set(ea[q][ea[q] >= 0].tolist())]
    assert differ, "the two summation orders agree on every query: the case shows nothing"


def test_c_entry_points_check_their_arguments_before_any_launch():
    from torchpq_amd import _lib
    lib = _lib.load()
    assert hasattr(lib, "tpq_ivfpq4_scan_topk") and hasattr(lib, "tpq_ivfpq4_scan_workspace_bytes")
    assert lib.tpq_ivfpq4_scan_workspace_bytes(100, 100, 1) == 0
    assert lib.tpq_ivfpq4_scan_workspace_bytes(100, 100, 3) == 100 * 3 * 2 * 64 * 8     # lists of 128 entries
    assert lib.tpq_ivfpq4_scan_workspace_bytes(100, 1025, 3) == 0 == lib.tpq_ivfpq4_scan_workspace_bytes(0, 10, 3)

    def scan(m=16, ds=2, nq=4, max_nprobe=2, k=10, metric=0, n_split=1, n_slots=100):
        return lib.tpq_ivfpq4_scan_topk(None, None, None, None, None, None, None, None, None, n_slots, m, ds, nq,
                                        max_nprobe, k, metric, n_split, None, 0, None)
    for bad_m in (0, 4, 12, 20, 257, 264, -8):
        assert scan(m=bad_m) == _lib.ERR_UNSUPPORTED and "m must be" in _lib.last_error(), bad_m
    assert scan(ds=0) == _lib.ERR_UNSUPPORTED
    for bad_k in (0, -1, 1025):
        assert scan(k=bad_k) == _lib.ERR_UNSUPPORTED and "k=" in _lib.last_error()
    assert scan(n_slots=2 ** 31 - 1) == _lib.ERR_UNSUPPORTED
    assert scan(metric=2) == -1 and scan(n_split=0) == -1 and scan(max_nprobe=0) == -1
    assert scan() == -1 and "null pointer" in _lib.last_error()        # a supported shape gets as far as the pointers
    assert scan(nq=0) == 0


def test_python_layers_decline_unsupported_shapes():
    from torchpq_amd.codec import PQ4Codec
    from torchpq_amd.kernels import IVFPQ4TopkHip
    for bad_m in (4, 12, 264):
        with pytest.raises(AssertionError):
            IVFPQ4TopkHip(m=bad_m)
    with pytest.raises(AssertionError):
        PQ4Codec(d_vector=30, n_subvectors=8)
    with pytest.raises(AssertionError):
        PQ4Codec(d_vector=30, n_subvectors=3)
    with pytest.raises(RuntimeError):
        from torchpq_amd.index import IVFPQ4Index
        IVFPQ4Index(32, 8, 16, device="cpu")
