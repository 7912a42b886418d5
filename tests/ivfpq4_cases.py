"""The list-scan cases of the IVFPQ4Index tests, shared by test_ivfpq4_cpu.py (what the inputs are) and
test_gpu_ivfpq4.py (the kernel on them); built like test_gpu_ivfflat._case."""
import numpy as np

import ivfpq4_oracle as porc

# cells of 0, 1, 63, 64, 65 and about 300 slots (and two more), each with spare capacity behind it
CELL_SIZES = (0, 1, 63, 64, 65, 300, 17, 128)

# the case whose summation order decides places: (seed, m, nq, n_probe, k)
OFFSET_CASE = (4242, 64, 3, 8, 10)


def case(seed, m, ds, nq, n_probe, tomb=25, dup=True, sizes=CELL_SIZES, offset=0.0):
    """`offset`: the codebook is offset + N(0,1), ds must be 1 and every query component is 1.0 -- with the inner
    product a table entry is then the codebook entry itself, exactly"""
    rng = np.random.default_rng(seed)
    sizes = np.array(sizes, np.int64)
    n_cells = len(sizes)
    caps = sizes + rng.integers(1, 9, n_cells)
    start = (np.cumsum(caps) - caps).astype(np.int64)
    cap = int(caps.sum())
    storage = rng.integers(0, 256, (m // 8, cap, 4), dtype=np.uint8)        # free slots hold junk codes
    codebook = rng.standard_normal((m, ds, 16)).astype(np.float32)
    query = rng.standard_normal((m * ds, nq)).astype(np.float32)
    if offset:
        assert ds == 1
        codebook = (codebook + np.float32(offset)).astype(np.float32)
        query[:] = 1.0
    is_empty = np.ones(cap, np.uint8)
    for c in range(n_cells):
        is_empty[start[c]:start[c] + sizes[c]] = 0
    live = np.flatnonzero(is_empty == 0)
    if dup:   # a third of the slots hold one of five codes: ties everywhere, the k-th place included
        src = rng.choice(live, 5, replace=False)
        dst = rng.choice(live, len(live) // 3, replace=False)
        storage[:, dst, :] = storage[:, src[rng.integers(0, 5, len(dst))], :]
    if tomb:
        is_empty[rng.choice(live, tomb, replace=False)] = 1
    cells = np.stack([rng.permutation(n_cells)[:n_probe] for _ in range(nq)])
    if n_probe > 1 and nq > 1:
        cells[1, 1] = cells[1, 0]                       # one cell listed twice in a row: scanned once
    npl = rng.integers(0, n_probe + 3, nq).astype(np.int64)   # below, at and beyond max_nprobe
    npl[:max(1, nq // 2)] = n_probe
    return dict(storage=storage, codebook=codebook, query=query, is_empty=is_empty, cs=start[cells], sz=sizes[cells],
                npl=npl)


def offset_case():
    seed, m, nq, n_probe, k = OFFSET_CASE
    return case(seed, m, 1, nq, n_probe, offset=-float(2 ** 20)), k


def pairwise_topk_sets(c, k, distance):
    """per query, the address set of the top-k (value descending, address ascending) when the m table entries are
    summed PAIRWISE in fp32 (a balanced tree) instead of the specification's ascending-j chain: a stand-in for
    "another summation order", not any kernel's own"""
    codes = porc.unpack(c["storage"])
    table = porc.lut(c["query"], c["codebook"], distance)
    m = codes.shape[0]
    out = []
    for q in range(c["query"].shape[1]):
        s = porc.probed_slots(c["cs"][q], c["sz"][q], c["npl"][q], codes.shape[1])
        s = s[c["is_empty"][s] == 0]
        t = table[q][np.arange(m)[:, None], codes[:, s]].T.astype(np.float32)   # [n, m]
        while t.shape[1] > 1:
            t = (t[:, 0::2] + t[:, 1::2]).astype(np.float32)                    # (m is a power of two here)
        order = np.lexsort((s, -t[:, 0].astype(np.float64)))[:k]
        out.append(set(s[order].tolist()))
    return out
