"""GPU: the fp16 list scan and range search (tpq_ivf_flat16_scan_topk / _range_count / _range_fill,
csrc/scan_flat_f16.hip) against the fp32 oracles on the rounded vectors, and IVFFlat16Index against an IVFFlatIndex
that holds x.half().float() -- every comparison bit for bit: values as int32 views, addresses and ids equal."""
import numpy as np
import pytest
import torch

import guarded_alloc
import ivfflat_f16_guarded
import ivfflat_f16_oracle as f16
import ivfflat_oracle as forc
import ivfflat_range_oracle as rorc
from tests_support import DEV, T, _clustered

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 130, 200)                            # the probed cells: around one tile, two, three and a bit
CELLS = np.array([[6, 6, 2, 4], [5, 3, 0, 1], [4, 2, 6, 5]])    # query 0 repeats a start; query 1 has 195 candidates


def _case(d, mask, planted):
    """`planted`: normal floats with +-0, 2^-24 (an fp16 subnormal) and 65504 among them; else integer components
    0 ... 218, exact in fp16 and full of ties.  mask "sparse": two live slots per tile, every tile below kCompactBelow"""
    rng = np.random.default_rng(100 * d + planted)
    sizes = np.array(SIZES, np.int64)
    start = (np.cumsum(sizes + 3) - sizes - 3).astype(np.int64)          # three spare slots behind every cell
    cap = int((sizes + 3).sum())
    if planted:
        x, q = rng.standard_normal((d, cap)).astype(np.float32), rng.standard_normal((d, 3)).astype(np.float32)
        x[rng.integers(0, d, 40), rng.integers(0, cap, 40)] = np.tile(np.float32([0.0, -0.0, 2.0 ** -24, 65504.0]), 10)
    else:
        x, q = (rng.integers(0, 219, s).astype(np.float32) for s in ((d, cap), (d, 3)))
    is_empty = {"none": None, "some": (rng.random(cap) < 0.3).astype(np.uint8)}.get(mask, np.ones(cap, np.uint8))
    if mask == "sparse":
        for c in range(len(sizes)):
            is_empty[start[c] + 5:start[c] + sizes[c]:32] = 0
    return dict(words=f16.pack(x).view(np.int32), vectors=f16.rounded(x), query=q, is_empty=is_empty, cs=start[CELLS],
                sz=sizes[CELLS], npl=np.full(3, 4, np.int64))


def _equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape
        assert torch.equal(g.view(torch.int32) if g.dtype == torch.float32 else g,
                           w.view(torch.int32) if w.dtype == torch.float32 else w)


@pytest.mark.parametrize("mask", ["none", "some", "sparse", "all"])
@pytest.mark.parametrize("distance", ["euclidean", "inner"])
@pytest.mark.parametrize("d", [1, 2, 15, 16, 17, 33])
def test_kernels_against_the_oracle(d, distance, mask):
    """top-k for k = 1, 10, 200 (pads) and the range passes at thresholds from the oracle's own values -- the 5th
    best, the smallest, +inf -- each with one and with three workgroups per query"""
    from torchpq_amd.kernels import IVFFlat16RangeHip, IVFFlat16TopkHip
    topk, ranged = IVFFlat16TopkHip(), IVFFlat16RangeHip()
    for planted in (False, True):
        case = _case(d, mask, planted)
        args = [case[n] for n in ("vectors", "query", "is_empty", "cs", "sz", "npl")]
        gpu = [T(case[n]) for n in ("words", "query", "cs", "sz", "npl")]
        kw = dict(is_empty=None if mask == "none" else T(case["is_empty"]), distance=distance)
        cand = rorc.candidates(*args, distance)
        ranked = [np.sort(v[~np.isnan(v)])[::-1] for _, v in cand]
        assert mask == "all" or min(len(v) for v in ranked) > 0
        for k in (1, 10, 200):
            want = forc.scan_topk(*args, k, distance)
            assert mask in ("sparse", "all") or ((want[1] >= 0).all() if k < 200 else (want[1][1] < 0).any())
            for n_split in (1, 3):
                _equal(topk(*gpu, k, n_split=n_split, **kw), [T(w) for w in want])
        for pick in (lambda v: v[min(4, len(v) - 1)], lambda v: v[-1], lambda v: np.inf):
            thr = np.float32([pick(v) if len(v) else 0.0 for v in ranked])
            want = rorc.range_scan(*args, thr, distance, cand=cand)
            for n_split in (1, 3):
                _equal(ranged(*gpu, T(thr), n_split=n_split, **kw), [T(w) for w in want])


def test_index_equals_ivfflat_on_the_rounded_vectors():
    from torchpq_amd.index import IVFFlat16Index, IVFFlatIndex
    d = 17
    base, queries = (T(t) for t in _clustered(5, d, 1500, 40))
    ref = IVFFlatIndex(d, n_cells=8, initial_size=64, device=DEV)
    ref.train(base)
    idx = IVFFlat16Index(d, n_cells=8, initial_size=64, device=DEV)
    idx.vq_codec.load_state_dict(ref.vq_codec.state_dict())
    for part in (base[:, :400], base[:, 400:]):                  # the second batch grows the cells
        ids = idx.add(part.contiguous())
        assert torch.equal(ids, ref.add(part.half().float().contiguous()))
    gone = torch.arange(0, 1500, 7, device=DEV)
    for index in (idx, ref):
        index.remove(ids=gone)
    assert idx._storage.numel() == 4 * ((d + 1) // 2) * idx.capacity and idx.capacity == ref.capacity
    fresh = IVFFlat16Index(d, n_cells=8, initial_size=64, device=DEV)
    fresh.load_state_dict(idx.state_dict())
    allowed = torch.arange(0, 1500, 3, device=DEV)
    for index in (idx, fresh):
        index.n_probe = ref.n_probe = 3
        index.use_cell_major, index.cell_major_min_batch = True, 1
        _equal(index.search(queries, k=100, return_address=True), ref.search(queries, k=100, return_address=True))
        assert index.last_route == "query_major"
        _equal(index.search_filtered(queries, 20, index.id_filter(allowed)),
               ref.search_filtered(queries, 20, ref.id_filter(allowed)))
        hits = index.range_search(queries, -30.0)
        assert 40 < int(hits[0][-1]) < 40 * 1500
        _equal(hits, ref.range_search(queries, -30.0))
        _equal([index.reconstruct(ids=allowed)], [ref.reconstruct(ids=allowed)])


def test_f16_inside_guarded_buffers(monkeypatch):
    """tests/ivfflat_f16_guarded.py between canaries: the guards hold, the same bits from 0x00- and 0xFF-filled buffers"""
    out = guarded_alloc.run_guarded(ivfflat_f16_guarded.build(), monkeypatch=monkeypatch)
    _equal(out[0x00], out[0xFF])
