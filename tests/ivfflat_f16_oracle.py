"""NumPy oracle of the fp16 list layout of IVFFlat16Index (include/torchpq_amd.h): pack and unpack only.  The scans are
tests/ivfflat_oracle.py / tests/ivfflat_range_oracle.py on `rounded(x)`: that is the value's definition."""
import numpy as np


def rounded(x):
    """f32 -> the f32 of its nearest-even fp16"""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def pack(x):
    """f32 [d, n] -> u32 [ceil(d / 2), n]: word r holds half(x[2 r]) in its low 16 bits and half(x[2 r + 1]) in its
    high 16 bits; the high half past an odd d is +0"""
    d, n = x.shape
    with np.errstate(over="ignore"):
        h = np.zeros((2 * ((d + 1) // 2), n), np.float16)
        h[:d] = np.asarray(x, np.float32).astype(np.float16)
    bits = h.view(np.uint16).astype(np.uint32)
    return bits[0::2] | (bits[1::2] << 16)


def unpack(words, d):
    """u32 [ceil(d / 2), n] -> f32 [d, n] of the stored halves"""
    rows, n = words.shape
    bits = np.empty((2 * rows, n), np.uint16)
    bits[0::2] = words & 0xFFFF
    bits[1::2] = words >> 16
    return bits.view(np.float16)[:d].astype(np.float32)

