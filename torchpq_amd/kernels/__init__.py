"""Kernel wrappers: torch tensors in, torch tensors out, HIP underneath.

Each class mirrors one CuPy RawKernel wrapper of the reference (torchpq/kernels/*Cuda.py):
same call signature and argument meaning, same asserts, outputs allocated with torch and
owned by the caller, launches asynchronous on the CURRENT torch stream, never synchronising.
There is no CPU path: tensors must live on the GPU.

One module per subsystem -- scan.py, coarse.py, kmeans.py, container.py, flat.py; what they share is in _common.py.
"""
from .coarse import (CoarseProbeHip, CoarseSelectHip, SmartProbingHip, Top1SelectHip, Top32SelectHip,
                     TopkSelectHip)
from .container import (GetAddressByIdHip, GetCellByAddressHip, GetIdByAddressHip, GetIOAHip,
                        GetWriteAddressHip, GrowCellsHip, PackCodesHip, PQDecodeHip, ScatterCodesHip)
from .flat import FlatRangeHip, FlatTopkHip
from .kmeans import ComputeCentroidsHip, CoarseAssignHip, LloydStepHip, MaxSimHip, MaxSimSelectHip
from .scan import (PACKED_M, AdcLutHip, CellCandidatesHip, CellKeptState, IVFFlatRangeHip, IVFFlatTopkHip, IVFPQ4FilteredTopkHip, IVFPQ4RangeHip, IVFPQ4ResidualTopkHip, IVFPQ4TopkHip, IVFPQFilteredTopkHip, IVFPQRangeHip,
                   IVFPQRerankHip, IVFPQTop1Hip, IVFPQTopkHip, ResidualPart1Hip, ResidualSlotTermsHip, ScanOrderHip, SlotFilterBuildHip,
                   packed_chunk_width)

__all__ = [
    "IVFPQTopkHip", "IVFPQTop1Hip", "ScanOrderHip", "CellCandidatesHip", "ResidualPart1Hip", "ResidualSlotTermsHip", "AdcLutHip", "TopkSelectHip", "CoarseSelectHip", "CoarseProbeHip", "Top1SelectHip",
    "Top32SelectHip", "SmartProbingHip", "MaxSimHip", "CoarseAssignHip", "MaxSimSelectHip", "LloydStepHip", "ComputeCentroidsHip", "GetIOAHip",
    "GetWriteAddressHip", "GetCellByAddressHip", "GetIdByAddressHip", "GetAddressByIdHip", "GrowCellsHip", "PQDecodeHip",
    "ScatterCodesHip", "PackCodesHip", "IVFPQRerankHip", "IVFFlatTopkHip", "IVFFlatRangeHip", "IVFPQ4TopkHip", "IVFPQ4ResidualTopkHip", "IVFPQ4FilteredTopkHip", "IVFPQ4RangeHip", "IVFPQRangeHip", "IVFPQFilteredTopkHip", "SlotFilterBuildHip", "FlatTopkHip", "FlatRangeHip", "packed_chunk_width", "PACKED_M", "CellKeptState",
]
