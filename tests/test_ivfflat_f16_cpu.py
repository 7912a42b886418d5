"""CPU: the C-ABI symbols of the fp16 list scan (declared, bound, their checks before any HIP call), the packed
layout of IVFFlat16Index against tests/ivfflat_f16_oracle.py, and the class's place next to IVFFlatIndex."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import ivfflat_f16_guarded  # noqa: F401  (registers the guarded case of the new entry points)
import ivfflat_f16_oracle as f16
import ivfflat_oracle as forc
from conftest import ROOT

#             vectors query empty start size npl [thr] out... n_slots d nq np [k] metric split [ws bytes] stream
TOPK = [None] * 8 + [100, 8, 1, 4, 10, 0, 1, None, 0, None]
COUNT = [None] * 8 + [100, 8, 1, 4, 0, 1, None]
FILL = [None] * 10 + [100, 8, 1, 4, 0, 1, None]


@pytest.mark.parametrize("symbol,args,first", [("tpq_ivf_flat16_scan_topk", TOPK, 8),
                                               ("tpq_ivf_flat16_range_count", COUNT, 8),
                                               ("tpq_ivf_flat16_range_fill", FILL, 10)])
def test_symbols_declared_bound_and_checked_before_any_hip_call(symbol, args, first):
    """the table of tests/test_ivfflat_cpu.py; `first`: the position of n_slots, then d, nq, max_nprobe, [k,] metric, n_split"""
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    assert re.search(r"\b%s\s*\(const uint32_t\* vectors" % symbol, header) and symbol in _lib.SIGNATURES
    assert "#define TPQ_HAS_IVFFLAT_F16 1" in header and "float(half(x))" in header
    fn = getattr(_lib.load(), symbol)
    assert fn(*args) == -1 and "null pointer" in _lib.last_error()
    has_k = symbol.endswith("topk")
    metric = first + 4 + has_k
    bad = [(first + 1, 0), (first + 3, 0), (metric, 2), (metric + 1, 0)] + ([(first + 4, 1025), (first + 4, 0)] * has_k)
    having = lambda pos, value: args[:pos] + [value] + args[pos + 1:]  # noqa: E731
    for pos, value in bad:
        assert fn(*having(pos, value)) == -1, (pos, value)
    assert fn(*having(first, (1 << 31) - 1)) == _lib.ERR_UNSUPPORTED and "2^31" in _lib.last_error()
    assert fn(*having(first + 2, 0)) == 0  # no queries: nothing to do


@pytest.mark.parametrize("d", [1, 2, 7])
def test_pack_unpack_round_trip(d):
    from torchpq_amd.index import IVFFlat16Index
    rng = np.random.default_rng(d)
    x = rng.standard_normal((d, 37)).astype(np.float32)
    x[0, :6] = [0.0, -0.0, 2.0 ** -24, 65504.0, 1e6, 1.0 + 2.0 ** -11]     # subnormal, max, overflow, a tie to even
    codes = IVFFlat16Index.vectors_to_codes(torch.from_numpy(x))
    words = f16.pack(x)
    assert codes.shape == (4 * ((d + 1) // 2), 37) and codes.dtype == torch.uint8 and words.shape == ((d + 1) // 2, 37)
    assert np.array_equal(codes.numpy(), forc.vectors_to_codes(words.view(np.float32)))   # byte b of word r: row 4 r + b
    want = f16.rounded(x)
    assert np.array_equal(words[0] & 0xFFFF, want[0].astype(np.float16).view(np.uint16))
    if d % 2:
        assert not (words[-1] >> 16).any()                     # the high half past an odd d is +0
    back = IVFFlat16Index.codes_to_vectors(codes, d)
    assert back.shape == (d, 37) and np.array_equal(back.numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(f16.unpack(words, d).view(np.uint32), want.view(np.uint32))
    assert np.isinf(want[0, 4]) and want[0, 5] == 1.0 and want[0, 2] == 2.0 ** -24


def test_class_is_exported_and_ivfflat_is_untouched():
    import torchpq_amd.index as index
    from torchpq_amd import kernels
    assert "IVFFlat16Index" in index.__all__ and {"IVFFlat16TopkHip", "IVFFlat16RangeHip"} <= set(kernels.__all__)
    assert issubclass(index.IVFFlat16Index, index.IVFFlatIndex) and index.IVFFlat16Index is not index.IVFFlatIndex
    # (tests/test_ivfflat_cpu.py pins IVFFlatIndex's own signature)
    assert inspect.signature(index.IVFFlat16Index.__init__) == inspect.signature(index.IVFFlatIndex.__init__)
    with pytest.raises(AssertionError):
        index.IVFFlat16Index(0, device="cpu")
    with pytest.raises(RuntimeError, match="GPU"):
        index.IVFFlat16Index(7, device="cpu")
