"""CPU restatement of the IVFPQRIndex re-rank step (TEST INFRASTRUCTURE ONLY; nothing under torchpq_amd/
imports it).  numpy fp32 in exactly the order include/torchpq_amd.h gives for tpq_ivfpqr_rerank; the first
stage is the existing oracle (oracle/ivfpq_oracle.py, oracle/c_oracle.py)."""
import numpy as np

from oracle import c_oracle
from oracle import ivfpq_oracle as orc

F32 = np.float32


def _codes(storage, rows, address):
    """codes [len(rows), n] of the slots `address` (all valid)"""
    return np.stack([storage[j // 4, address, j % 4] for j in rows])


def decode_sum(codebook, codebook_r, c, c_r):
    """decode(c) + decode_r(c_r), one fp32 add per component: [d, n]"""
    return (orc.pq_decode(codebook, c) + orc.pq_decode(codebook_r, c_r)).astype(F32)


def rerank_values(storage, codebook, codebook_r, query, address, use_residual, distance):
    """value of candidate `address[q, c]` (all valid slots) for query q: f32 [nq, k1]"""
    nq, k1 = address.shape
    m_r, ds_r, _ = codebook_r.shape
    m = storage.shape[0] * 4 - m_r
    d = m_r * ds_r
    flat = address.reshape(-1)
    c_r = _codes(storage, range(m, m + m_r), flat)
    if not use_residual:
        lut = c_oracle.adc_lut(query, codebook_r, distance)          # [m_r, nq, 256], tpq_adc_lut's arithmetic
        qi = np.repeat(np.arange(nq), k1)
        v = np.zeros(flat.shape[0], dtype=F32)
        for j in range(m_r):
            v = (v + lut[j, qi, c_r[j]]).astype(F32)
        return v.reshape(nq, k1)
    ds = d // m
    c = _codes(storage, range(m), flat)
    q = np.repeat(np.ascontiguousarray(query, dtype=F32), k1, axis=1)  # [d, nq * k1]
    acc = np.zeros(flat.shape[0], dtype=F32)
    for i in range(d):
        r = (codebook[i // ds, i % ds, c[i // ds]] + codebook_r[i // ds_r, i % ds_r, c_r[i // ds_r]]).astype(F32)
        if distance == "euclidean":
            t = (q[i] - r).astype(F32)
            acc = (acc - (t * t).astype(F32)).astype(F32)
        else:
            acc = (acc + (q[i] * r).astype(F32)).astype(F32)
    return acc.reshape(nq, k1)


def rerank(storage, codebook, codebook_r, query, cand_address, k, use_residual=True, distance="euclidean",
           address2id=None):
    """The k best of each query's candidates by (value descending, address ascending); candidates outside
    [0, capacity) are none; unfilled positions (-inf, -1, -1).  Returns (values, address, ids)."""
    storage = np.asarray(storage)
    cand_address = np.asarray(cand_address, dtype=np.int64)
    nq, k1 = cand_address.shape
    cap = storage.shape[1]
    real = (cand_address >= 0) & (cand_address < cap)
    v = rerank_values(storage, None if codebook is None else np.asarray(codebook, dtype=F32),
                      np.asarray(codebook_r, dtype=F32), query, np.where(real, cand_address, 0), use_residual,
                      distance)
    vals = np.full((nq, k), -np.inf, dtype=F32)
    adr = np.full((nq, k), -1, dtype=np.int64)
    for q in range(nq):
        pos = np.nonzero(real[q])[0]
        order = pos[np.lexsort((pos, cand_address[q, pos], -v[q, pos]))][:k]
        vals[q, :order.size] = v[q, order]
        adr[q, :order.size] = cand_address[q, order]
    ids = None if address2id is None else orc.get_id_by_address(np.asarray(address2id), adr)
    return vals, adr, ids


def search(x, pq_codebook, pq_codebook_r, storage, is_empty, cell_start, cell_size, address2id, cells, n_probe_list,
           k, rerank_factor, use_residual=True, distance="euclidean"):
    """IVFPQRIndex.search after the coarse step (`cells` [nq, n_probe], `n_probe_list` [nq] come from the
    index): the existing oracle's list scan over the first-stage rows at k1 = k * rerank_factor, then
    rerank().  `x` is already normalised for "cosine".  Returns (values, ids, address)."""
    m = pq_codebook.shape[0]
    lut = c_oracle.adc_lut(x, pq_codebook, distance)
    _, cand = c_oracle.scan_topk(np.ascontiguousarray(storage[:m // 4]), lut, is_empty, cell_start[cells],
                                 cell_size[cells], n_probe_list, k * rerank_factor)
    vals, adr, ids = rerank(storage, pq_codebook, pq_codebook_r, x, cand, k, use_residual, distance, address2id)
    return vals, ids, adr
