"""numpy model of the cell-major candidate arithmetic (csrc/scan_cells.hip), float64 throughout, no torch.

The kernel scales query and codebook by powers of two so that the largest scaled component lies in [2^12, 2^13), splits
every scaled component y into two fp16 pieces h = fp16(y), l = fp16(y - h), and accumulates the three products
xl.qh + xh.ql + xh.qh on the fp16 matrix cores in fp32.  This module computes, per (query, slot):

  exact   the metric in float64 on the unsplit fp32 data;
  model   the value the kernel aims at, in float64 from the pieces;
  T       sum |terms| over the three products (scaled units);
  tol     the per-slot rounding allowance of the kernel against `model`: the header's "fp32 accumulation", "norm chains"
          and "two subtractions" lines evaluated for the slot instead of being bounded by B^2;
  emu     a deterministic fp32 emulation of the accumulation, the three products of a k-step in the kernel's order;

and per query delta_q = delta_rel(ds) B^2, the kernel's documented selection band, B = |q| + sqrt(sum_j max_c |c_jc|^2).

Layouts: codebook [64, ds, 256] fp32, query [64 ds, nq] fp32 (component i = j ds + e), codes [n_slots, 64] uint8,
storage [16, n_slots, 4] uint8 with sub-quantizer j = 4 g + b at storage[g, slot, b]."""
import numpy as np

M = 64
SCALE_EXP = 12      # kCellScaleExp: the largest scaled magnitude lies in [2^12, 2^13)
MAX_EXP = 40        # kCellMaxExp
F16_MIN_NORMAL = 2.0 ** -14
U24, U23, U22 = 2.0 ** -24, 2.0 ** -23, 2.0 ** -22
METRICS = ("euclidean", "inner")


# ---- the split and the scales ---------------------------------------------------------------------------------------
def split(y, flush=False):
    """h = fp16(y), l = fp16(y - h), both round-to-nearest-even, y an fp32 array; returned as float64.  `flush`: pieces
    below the fp16 normal range become zero (the other behaviour the hardware may choose)."""
    y = np.asarray(y, np.float32)
    h = y.astype(np.float16)
    if flush:
        h = np.where(np.abs(h.astype(np.float64)) < F16_MIN_NORMAL, np.float16(0), h)
    l = (y - h.astype(np.float32)).astype(np.float32).astype(np.float16)
    if flush:
        l = np.where(np.abs(l.astype(np.float64)) < F16_MIN_NORMAL, np.float16(0), l)
    return h.astype(np.float64), l.astype(np.float64)


def scale_of(maxabs):
    """the power of two s with s * maxabs in [2^12, 2^13); maxabs > 0 (array or scalar)"""
    _, e = np.frexp(np.asarray(maxabs, np.float64))   # maxabs = f 2^e, f in [0.5, 1): floor(log2) = e - 1
    return np.ldexp(1.0, SCALE_EXP - (e - 1))


def ulp_fp16(h):
    """spacing of the fp16 numbers at the normal fp16 value h"""
    _, e = np.frexp(np.abs(np.asarray(h, np.float64)))
    return np.ldexp(1.0, e - 1 - 10)


def decode(codebook, codes):
    """[n_slots, 64 ds] fp32: the decoded slots"""
    m, ds, _ = codebook.shape
    return codebook[np.arange(m)[None, :], :, codes.astype(np.int64)].reshape(codes.shape[0], m * ds)


def storage_of(codes):
    """[16, n_slots, 4] uint8, the container's layout"""
    return np.ascontiguousarray(codes.reshape(codes.shape[0], M // 4, 4).transpose(1, 0, 2))


# ---- the bound the kernel documents ---------------------------------------------------------------------------------
def header_terms(ds):
    """the lines of the header's error budget, relative to B^2, in float64"""
    D = 64.0 * ds
    N = 3.0 * D
    return {
        "dropped product, residues, fp32 accumulation": 0.5 * (3.03 * U22 + 1.003 * N * U23),
        "subnormal pieces": 1.01 * np.sqrt(D) * 2.0 ** -26,
        "norm chains": (D + 1) * U24,
        "|x|^2 from the pieces": 14 * U24,
        "two subtractions, tau - delta": U22,
        "exact chain": 1.001 * (M + ds + 2) * U24,
    }


def delta_rel(ds):
    """delta_q / B^2 as the header documents it: 1.25 x the sum of its terms"""
    return 1.25 * sum(header_terms(ds).values())


def bound_B(query, codebook):
    """[nq] float64: B = |q| + |x|max, |x|max^2 = sum_j max_c |c_jc|^2"""
    q = np.asarray(query, np.float64)
    cb = np.asarray(codebook, np.float64)
    return np.sqrt((q * q).sum(0)) + np.sqrt((cb * cb).sum(1).max(1).sum())


def delta_q(query, codebook):
    ds = codebook.shape[1]
    return delta_rel(ds) * bound_B(query, codebook) ** 2


# ---- exact, model, tolerance ----------------------------------------------------------------------------------------
def exact(q, x, metric="euclidean"):
    """[nq, n] float64 on the unsplit data; q [nq, D], x [n, D]"""
    q, x = np.asarray(q, np.float64), np.asarray(x, np.float64)
    dot = q @ x.T
    if metric == "inner":
        return dot
    # -(|q|^2 - 2 q.x + |x|^2) loses digits when q is close to x: the difference is taken per component
    out = np.empty((q.shape[0], x.shape[0]))
    for i in range(q.shape[0]):
        d = x - q[i]
        out[i] = -(d * d).sum(1)
    return out


def evaluate(query, codebook, codes, metric="euclidean", flush=False, emulate=False):
    """everything the tests compare, for every (query, slot): dict of [nq, n] float64 arrays exact, model, T, tol
    (and emu when asked), [nq] delta, and the scales"""
    ds = codebook.shape[1]
    D = M * ds
    q32 = np.ascontiguousarray(np.asarray(query, np.float32).T)                 # [nq, D]
    x32 = decode(np.asarray(codebook, np.float32), codes)                       # [n, D]
    sx = float(scale_of(np.abs(codebook).max()))
    sq = scale_of(np.abs(q32).max(1))                                           # [nq]
    xh, xl = split((x32.astype(np.float64) * sx).astype(np.float32), flush)
    qh, ql = split((q32.astype(np.float64) * sq[:, None]).astype(np.float32), flush)
    S = qh @ xh.T + ql @ xh.T + qh @ xl.T
    T = np.abs(qh) @ np.abs(xh).T + np.abs(ql) @ np.abs(xh).T + np.abs(qh) @ np.abs(xl).T
    unscale = 1.0 / (sq[:, None] * sx)
    X2 = ((xh + xl) ** 2).sum(1)[None, :] / (sx * sx)
    Q2 = (q32.astype(np.float64) ** 2).sum(1)[:, None]
    if metric == "inner":
        model = S * unscale
        tol = 1.003 * 3 * D * U23 * T * unscale
    else:
        model = 2 * S * unscale - X2 - Q2
        tol = (1.003 * 3 * D * U23 * 2 * T * unscale + (D + 1) * U24 * (X2 + Q2)
               + U23 * (2 * T * unscale + X2 + Q2))
    out = dict(exact=exact(q32, x32, metric), model=model, T=T, tol=tol, delta=delta_q(query, codebook), sx=sx, sq=sq,
               X2=X2, Q2=Q2)
    if emulate:
        out["emu"] = _emulate(xh, xl, qh, ql, q32, sx, sq, metric)
    return out


def _emulate(xh, xl, qh, ql, q32, sx, sq, metric):
    """fp32 throughout: per k-step of 16 components the products xl qh, xh ql, xh qh, each added to the accumulator one
    term at a time (a product of two fp16 numbers is exact in fp32); |x|^2 as two fma-like chains over the halves of
    every k-step, added; |q|^2 an fp32 sum; 2 dot - |x|^2 - |q|^2 in the kernel's order"""
    f = np.float32
    nq, D = qh.shape
    n = xh.shape[0]
    acc = np.zeros((nq, n), f)
    xh32, xl32, qh32, ql32 = (a.astype(f) for a in (xh, xl, qh, ql))
    for s in range(D // 16):
        for a, b in ((xl32, qh32), (xh32, ql32), (xh32, qh32)):
            for i in range(16 * s, 16 * s + 16):
                acc = (acc + (b[:, i:i + 1] * a[None, :, i]).astype(f)).astype(f)
    dot = (acc.astype(np.float64) / (sq[:, None] * sx)).astype(f)               # (powers of two: exact)
    if metric == "inner":
        return dot.astype(np.float64)
    v = (xh32 + xl32).astype(f)
    chains = [np.zeros(n, f), np.zeros(n, f)]
    for s in range(D // 16):
        for half in (0, 1):
            for i in range(16 * s + 8 * half, 16 * s + 8 * half + 8):
                # (the fma rounds once: the square is taken in float64, where it is exact)
                chains[half] = (chains[half].astype(np.float64) + v[:, i].astype(np.float64) ** 2).astype(f)
    x2 = ((chains[0] + chains[1]).astype(f).astype(np.float64) / (sx * sx)).astype(f)
    q2 = np.zeros(nq, f)
    for i in range(D):
        q2 = (q2.astype(np.float64) + q32[:, i].astype(np.float64) ** 2).astype(f)
    return (((f(2) * dot).astype(f) - x2[None, :]).astype(f) - q2[:, None]).astype(f).astype(np.float64)


# ---- the input families ---------------------------------------------------------------------------------------------
FAMILIES = ("random", "coherent", "coherent_lo", "one_subq", "near", "wide", "scaled", "scaled_rev")
# (`scaled`: the codebook times 2^40, the query times 1.9 2^-40; `scaled_rev`: the other way round)


def _lo(rng, shape):
    """positive values y / 2^12 whose scaled image y is h + r ulp_fp16(h), h an fp16 number in [2^10, 4304], r drawn per
    component from (0.05, 0.45): the low piece is large, of one sign and differs from component to component.  (4304 <
    2^13 / 1.9: `scaled` may multiply by 1.9 without leaving the binade of the largest component.)"""
    h = rng.uniform(1024.0, 4304.0, shape).astype(np.float16).astype(np.float64)
    y = h + rng.uniform(0.05, 0.45, shape) * ulp_fp16(h)
    return (y / 4096.0).astype(np.float32)


def _lo_top(rng, shape):
    """the same with h in [2^12, 4304]: a component that pins the scale"""
    h = rng.uniform(4096.0, 4304.0, shape).astype(np.float16).astype(np.float64)
    y = h + rng.uniform(0.05, 0.45, shape) * ulp_fp16(h)
    return (y / 4096.0).astype(np.float32)


def family(name, ds, nq, n_slots, seed=0):
    """-> codebook [64, ds, 256] fp32, query [64 ds, nq] fp32, codes [n_slots, 64] uint8; seeded, deterministic"""
    assert name in FAMILIES, name
    rng = np.random.default_rng([seed, FAMILIES.index(name), ds])
    D = M * ds
    codes = rng.integers(0, 256, (n_slots, M), dtype=np.uint8)
    if name == "random":
        cb = (rng.standard_normal((M, ds, 256)) * 3).astype(np.float32)
        q = (rng.standard_normal((D, nq)) * 3).astype(np.float32)
    elif name == "coherent":
        cb = rng.uniform(1.0, 1.25, (M, ds, 256)).astype(np.float32)
        q = rng.uniform(1.0, 1.25, (D, nq)).astype(np.float32)
    elif name in ("coherent_lo", "scaled", "scaled_rev"):
        cb, q = _lo(rng, (M, ds, 256)), _lo(rng, (D, nq))
        cb[rng.integers(M), rng.integers(ds), rng.integers(256)] = _lo_top(rng, ())
        q[rng.integers(0, D, nq), np.arange(nq)] = _lo_top(rng, nq)
        if name != "coherent_lo":
            up, down = np.float32(2.0 ** 40), np.float32(2.0 ** -40)
            cb, q = (cb * up, q * np.float32(1.9) * down) if name == "scaled" else (cb * down, q * np.float32(1.9) * up)
    elif name == "one_subq":
        assert nq == M, "one query per sub-quantizer"
        cb = _lo(rng, (M, ds, 256))
        cb[rng.integers(M), rng.integers(ds), rng.integers(256)] = _lo_top(rng, ())
        q = np.zeros((D, nq), np.float32)
        for j in range(M):
            q[j * ds:(j + 1) * ds, j] = _lo(rng, ds)
            q[j * ds + rng.integers(ds), j] = _lo_top(rng, ())
    elif name == "near":
        cb = (rng.standard_normal((M, ds, 256)) * 3).astype(np.float32)
        x = decode(cb, codes)
        q = (x[rng.integers(0, n_slots, nq)].astype(np.float64) * (1 + 2.0 ** -12)).astype(np.float32).T
    else:  # wide
        mag = lambda shape: (np.exp2(rng.uniform(-30.0, 0.0, shape)) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)  # noqa: E731
        cb, q = mag((M, ds, 256)), mag((D, nq))
    return np.ascontiguousarray(cb), np.ascontiguousarray(q), codes
