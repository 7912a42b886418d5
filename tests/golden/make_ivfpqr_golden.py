"""Writes tests/golden/fx_ivfpqr_pin.npz: inputs of the IVFPQR re-rank value and what the reference's own
Python computes for them on the CPU (PQCodec._decode_cpu of both codes, their sum, and the reference's metric
functions between queries and the sum).  Arrays only.  Needs the reference tree (oracle/_refimport.py):

    python tests/golden/make_ivfpqr_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def make_inputs(seed=7, d=32, m=8, m_r=16, n=96, nq=5):
    rng = np.random.default_rng(seed)
    codebook = rng.standard_normal((m, d // m, 256)).astype(np.float32)
    codebook_r = (0.25 * rng.standard_normal((m_r, d // m_r, 256))).astype(np.float32)
    codes = rng.integers(0, 256, (m, n), dtype=np.uint8)
    codes_r = rng.integers(0, 256, (m_r, n), dtype=np.uint8)
    query = rng.standard_normal((d, nq)).astype(np.float32)
    query_unit = (query / np.linalg.norm(query, axis=0, keepdims=True)).astype(np.float32)
    return dict(codebook=codebook, codebook_r=codebook_r, codes=codes, codes_r=codes_r, query=query,
                query_unit=query_unit)


def reference_results(inp):
    """the reference's decode of both codes, their sum, and its two metrics against the sum"""
    import torch
    from oracle import _refimport
    torchpq = _refimport.import_reference()
    dec = torchpq.codec.PQCodec._decode_cpu
    a = dec(torch.from_numpy(inp["codebook"]), torch.from_numpy(inp["codes"]))
    b = dec(torch.from_numpy(inp["codebook_r"]), torch.from_numpy(inp["codes_r"]))
    recon = a + b
    l2 = torchpq.metric.negative_squared_l2_distance(torch.from_numpy(inp["query"]), recon)
    dot = torchpq.metric.cosine_similarity(torch.from_numpy(inp["query_unit"]), recon, normalize=False)
    return dict(ref_recon=recon.numpy(), ref_l2=l2.numpy(), ref_dot=dot.numpy())


if __name__ == "__main__":
    inputs = make_inputs()
    out = dict(inputs, **reference_results(inputs))
    path = os.path.join(HERE, "fx_ivfpqr_pin.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
