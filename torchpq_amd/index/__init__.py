"""Index classes: the IVFPQ drop-in, its two-stage (re-rank) variant, its 4-bit variant, the IVF index over the stored vectors
themselves, the exact
(flat) index used as recall ground truth, and the
HIP-graph replay helper for fixed-shape serving batches."""
from . import FlatIndex as _flat_module
from . import IVFFlatIndex as _ivfflat_module
from . import IVFPQ4Index as _ivfpq4_module
from . import IVFPQIndex as _ivfpq_module
from . import IVFPQRIndex as _ivfpqr_module
from . import graphed as _graphed_module

IVFPQIndex = _ivfpq_module.IVFPQIndex
IVFPQRIndex = _ivfpqr_module.IVFPQRIndex
IVFPQ4Index = _ivfpq4_module.IVFPQ4Index
FlatIndex = _flat_module.FlatIndex
IVFFlatIndex = _ivfflat_module.IVFFlatIndex
GraphedSearch = _graphed_module.GraphedSearch

__all__ = ["IVFPQIndex", "IVFPQRIndex", "IVFPQ4Index", "IVFFlatIndex", "FlatIndex", "GraphedSearch"]
