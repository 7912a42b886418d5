"""CPU: the C-ABI symbols of the fp16 lists' cell-major scan -- declared, bound, their checks before any HIP call -- the
workspace size, and the wrapper's place in the package."""
import os
import re

import ivfflat_f16_cells_guarded  # noqa: F401  (registers the guarded case of the new entry point)
from conftest import ROOT

#       vectors ... out_addr  n_slots n_cells d nq np k metric first_probe cand_cap ws bytes stream
ARGS = [None] * 9 + [100, 4, 8, 1, 4, 10, 0, 2, 64, None, 0, None]
N_SLOTS, N_CELLS, D, NQ, NP, K, METRIC, P0, CAP = range(9, 18)


def test_symbols_declared_bound_and_checked_before_any_hip_call():
    from torchpq_amd import _lib
    header = open(os.path.join(ROOT, "include", "torchpq_amd.h")).read()
    assert "#define TPQ_HAS_IVFFLAT_F16_CELLS 1" in header
    for symbol in ("tpq_ivf_flat16_cells_topk", "tpq_ivf_flat16_cells_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % symbol, header) and symbol in _lib.SIGNATURES
    fn = _lib.load().tpq_ivf_flat16_cells_topk
    having = lambda pos, value: ARGS[:pos] + [value] + ARGS[pos + 1:]  # noqa: E731
    assert fn(*ARGS) == -1 and "null pointer" in _lib.last_error()
    for pos, value in ((N_CELLS, 0), (D, 0), (NP, 0), (K, 0), (METRIC, 2), (P0, 0), (NQ, -1)):
        assert fn(*having(pos, value)) == -1, (pos, value)
    for pos, value in ((D, 12), (D, 17), (K, 257), (CAP, 0), (CAP, 96), (N_SLOTS, (1 << 31) - 1)):
        assert fn(*having(pos, value)) == _lib.ERR_UNSUPPORTED, (pos, value)
    assert fn(*having(NQ, 0)) == 0  # no queries: nothing to do


def test_workspace_size():
    from torchpq_amd import _lib
    size = _lib.load().tpq_ivf_flat16_cells_workspace_bytes     # (nq, max_nprobe, n_cells, k, cand_cap, first_probe)
    for refused in ((0, 8, 16, 10, 64, 2), (10, 0, 16, 10, 64, 2), (10, 8, 0, 10, 64, 2), (10, 8, 16, 257, 64, 2),
                    (10, 8, 16, 10, 96, 2), (10, 8, 16, 10, 64, 0)):
        assert size(*refused) == 0, refused
    base = size(100, 8, 16, 10, 64, 2)
    assert base > 0 and base % 256 == 0
    assert size(100, 8, 16, 10, 128, 2) - base == 100 * 64 * 4      # the candidate lists: nq x cand_cap words
    # the fp32 route's regions and one more word per query: the scale exponent
    assert base == _lib.load().tpq_ivf_flat_cells_workspace_bytes(100, 8, 16, 10, 64, 2) + 512


def test_wrapper_is_exported():
    from torchpq_amd import kernels
    assert "IVFFlat16CellTopkHip" in kernels.__all__
    assert issubclass(kernels.IVFFlat16CellTopkHip, kernels.IVFFlatCellTopkHip)
    assert isinstance(kernels.IVFFlat16CellTopkHip().query_major, kernels.IVFFlat16TopkHip)
