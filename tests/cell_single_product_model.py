"""numpy model of the cell-major scan's single-product selection key (csrc/scan_cells.hip, `The single-product key`),
float64 throughout, no torch; the split, the scales and the input families are tests/scan_cells_oracle.py's.

The key keeps one of the three fp16 products: S1 = sum over the k-steps of xh.qh.  What it drops -- xh.ql + xl.qh + xl.ql --
is bounded per sub-quantizer j from XH_j = max_c |hi piece of s_x c_jc| and XL_j = max_c |lo piece| (the codebook's, kept in
the parameter block per PAIR of sub-quantizers, as the upper 16 bits of an fp32 rounded up) and the norms of the query's
pieces per sub-quantizer.  Per query
  delta1_q = 1.25 x ( (2 / (s_q s_x)) sum_j (XH_j |ql_j| + XL_j |qh_j| + XL_j |ql_j|)  +  the other lines x B^2 )."""
import numpy as np

import scan_cells_oracle as O

M = O.M
U24, U23, U22 = O.U24, O.U23, O.U22


def header_terms1(ds):
    """the lines of the single-product budget that are relative to B^2 (the dropped products are the query's own term)"""
    D = 64.0 * ds
    N = D
    return {
        "piece residues, fp32 accumulation": 0.5 * (2.03 * U22 + 1.003 * N * U23),
        "subnormal pieces": 1.01 * np.sqrt(D) * 2.0 ** -26,
        "norm chains": (D + 1) * U24,
        "|x|^2 from the pieces": 14 * U24,
        "two subtractions, tau - delta": U22,
        "exact chain": 1.001 * (M + ds + 2) * U24,
    }


def delta1_rel(ds):
    return 1.25 * sum(header_terms1(ds).values())


def pieces(query, codebook, flush=False):
    """the scaled split of both sides: dict of sx, sq [nq], cb_h / cb_l [64, ds, 256], qh / ql [nq, 64 ds]"""
    q32 = np.ascontiguousarray(np.asarray(query, np.float32).T)
    cb = np.asarray(codebook, np.float32)
    sx = float(O.scale_of(np.abs(cb).max()))
    sq = O.scale_of(np.abs(q32).max(1))
    cb_h, cb_l = O.split((cb.astype(np.float64) * sx).astype(np.float32), flush)
    qh, ql = O.split((q32.astype(np.float64) * sq[:, None]).astype(np.float32), flush)
    return dict(sx=sx, sq=sq, cb_h=cb_h, cb_l=cb_l, qh=qh, ql=ql, q32=q32)


def piece_maxima(p):
    """XH_j, XL_j [64] float64, exact: the largest norm of a sub-quantizer's hi (lo) pieces over its 256 entries"""
    return np.sqrt((p["cb_h"] ** 2).sum(1).max(1)), np.sqrt((p["cb_l"] ** 2).sum(1).max(1))


def round_up_16(v):
    """the kernel's 16-bit image of a positive number: the upper half of the fp32 of v x 1.0001, rounded up"""
    bits = (np.asarray(v, np.float64) * 1.0001).astype(np.float32).view(np.uint32).astype(np.uint64)
    return (((bits + 0xffff) >> 16) << 16).astype(np.uint32).view(np.float32).astype(np.float64)


def packed_maxima(XH, XL):
    """what the parameter block holds, expanded to [64] again: per pair of sub-quantizers the larger, rounded up"""
    pair = lambda X: np.repeat(round_up_16(X.reshape(32, 2).max(1)), 2)  # noqa: E731
    return pair(XH), pair(XL)


def dropped_bound(p, XH, XL):
    """[nq] float64, value units (x 2 / (s_q s_x), either metric): the bound on the three dropped products"""
    ds = p["cb_h"].shape[1]
    nq = p["qh"].shape[0]
    nh = np.sqrt((p["qh"].reshape(nq, M, ds) ** 2).sum(2))
    nl = np.sqrt((p["ql"].reshape(nq, M, ds) ** 2).sum(2))
    t = (XH[None, :] * nl + XL[None, :] * (nh + nl)).sum(1)
    return 2.0 * t / (p["sq"] * p["sx"])


def delta1_q(query, codebook, packed=False, flush=False):
    """[nq] float64: the single-product band of every query, from exact maxima or from the packed ones"""
    p = pieces(query, codebook, flush)
    XH, XL = piece_maxima(p)
    if packed:
        XH, XL = packed_maxima(XH, XL)
    ds = np.asarray(codebook).shape[1]
    return 1.25 * dropped_bound(p, XH, XL) + delta1_rel(ds) * O.bound_B(query, codebook) ** 2


def evaluate1(query, codebook, codes, metric="euclidean", flush=False):
    """per (query, slot), [nq, n] float64: exact; key -- the single-product key in float64 from the pieces --; dropped --
    the three dropped products in value units, as the kernel's scale has them (x 2 for the euclidean metric) --; tol --
    the fp32 roundings of the kernel against `key` (accumulation over N = D terms, norm chains, subtractions), per slot"""
    p = pieces(query, codebook, flush)
    ds = p["cb_h"].shape[1]
    D = M * ds
    codes = np.asarray(codes).astype(np.int64)
    xh = p["cb_h"][np.arange(M)[None, :], :, codes].reshape(codes.shape[0], D)
    xl = p["cb_l"][np.arange(M)[None, :], :, codes].reshape(codes.shape[0], D)
    x32 = O.decode(np.asarray(codebook, np.float32), codes)
    qh, ql = p["qh"], p["ql"]
    unscale = 1.0 / (p["sq"][:, None] * p["sx"])
    S1 = qh @ xh.T
    T1 = np.abs(qh) @ np.abs(xh).T
    drop = ql @ xh.T + qh @ xl.T + ql @ xl.T
    X2 = ((xh + xl) ** 2).sum(1)[None, :] / (p["sx"] ** 2)
    Q2 = (p["q32"].astype(np.float64) ** 2).sum(1)[:, None]
    if metric == "inner":
        key, dropped = S1 * unscale, drop * unscale
        tol = 1.003 * D * U23 * T1 * unscale
    else:
        key, dropped = 2 * S1 * unscale - X2 - Q2, 2 * drop * unscale
        tol = 1.003 * D * U23 * 2 * T1 * unscale + (D + 1) * U24 * (X2 + Q2) + U23 * (2 * T1 * unscale + X2 + Q2)
    return dict(exact=O.exact(p["q32"], x32, metric), key=key, dropped=dropped, tol=tol, p=p)
