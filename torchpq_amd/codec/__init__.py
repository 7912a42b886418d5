"""Quantisers: coarse inverted-file VQ, 8-bit and 4-bit product quantisers."""
from .BaseCodec import BaseCodec
from .PQ4Codec import PQ4Codec
from .PQCodec import PQCodec
from .VQCodec import VQCodec

__all__ = ["BaseCodec", "PQCodec", "PQ4Codec", "VQCodec"]
