"""GPU: candidate blocks dealt in pieces (csrc/scan_cells.h, kCellPiecesA / kCellPiecesB: piece i of S covers tiles
[i nt / S, (i + 1) nt / S) of a cell's nt = ceil(size / 32) tiles) against the reference-layout kernel (`packed=None`),
values bit for bit and addresses entry for entry, in the threshold form and in the seeded form.
The cells are the lengths at which a piece begins, ends or is empty -- 1, 31, 32, 33, 63, 64, 65, 32 S - 1, 32 S, 32 S + 1
for S = 2 and S = 4, and 1 025 -- among five long ones that keep the gate's mean of 512 slots (703 here, so that k = 128
takes the threshold form too), with a tombstone on the first and on the last row of every piece at S = 2 and at S = 4.
The file tests the library that is loaded.  The product build is A = 2, B = 1: under it the threshold form's first pass
runs in two pieces and the candidates proper run UNDIVIDED -- the flush per piece of pass B and the seeded form's pieces
are compiled out, and a suite run does not exercise them.  They, and S = 4 for either pass, are exercised only when this
file is run by hand against a tools/build_variant.sh build of scan_cells with -DTPQ_CELL_PIECES_A=s -DTPQ_CELL_PIECES_B=s
named by TPQ_AMD_LIB, s = 1, 2, 4 (done once, when S was chosen: profiles/cell_pieces_bench.json); nothing in the
repository repeats that run."""
import pytest
import torch

from test_gpu_scan_cell_threshold import _check, _gate
from test_gpu_scan_cells import DEV, _problem, _search
from test_scan_cell_maxima_cpu import G, T

pytestmark = pytest.mark.gpu

SIZES = [1, 1900, 31, 32, 1800, 33, 63, 64, 2000, 65, 127, 128, 1850, 129, 1025, 1950]
LONG = [c for c, sz in enumerate(SIZES) if sz >= 1800]
N_CELLS, N_PROBE = 16, 12


def _pieces_problem(seed, nq, ds, ragged, long_first=False):
    p = _problem(seed, nq, N_CELLS, N_PROBE, ds, sizes=SIZES, ragged=ragged)
    if long_first:
        # k >= 100: a query's first three probes are long cells, the others drawn from the remaining thirteen.  A query
        # with at least k maxima then has them from >= 56 tiles per probe, and its threshold admits a few hundred rows
        # -- not the better part of its probes, as the k-th of barely k maxima would, which overflows the lists and
        # sends a query outside the set below to the exact redo
        g = torch.Generator(device=DEV)
        g.manual_seed(seed)
        score = torch.rand(nq, N_CELLS, generator=g, device=DEV)
        pick = torch.tensor(LONG, device=DEV)[torch.rand(nq, len(LONG), generator=g, device=DEV).argsort(1)[:, :3]]
        score.scatter_(1, pick, score.gather(1, pick) - 2.0)
        p["cells"] = score.argsort(1)[:, :N_PROBE].contiguous()
    if ragged:
        p["npl"][:8] = torch.tensor([0, 1, T - 1, T, T + 1, N_PROBE, 2, N_PROBE], device=DEV)
    # a tombstone on the first and the last row of every piece, S = 2 and S = 4
    for c, (st, sz) in enumerate(zip(p["start"].tolist(), SIZES)):
        nt = (sz + 31) // 32
        for s in (2, 4):
            for i in range(s + 1):
                for row in (i * nt // s * 32 - 1, i * nt // s * 32):
                    if 0 <= row < sz:
                        p["is_empty"][st + row] = 1
        p["is_empty"][st + sz - 1] = 1
    return p


def _few_maxima(p, k):
    """queries whose first T probes can reserve fewer than k maxima -- the only ones that may be redone exactly (their
    threshold is -inf, and every live row of their probes need not fit the lists); from the sizes alone"""
    tiles = (p["sizes"][p["cells"]] + 31) // 32
    listed = torch.arange(N_PROBE, device=DEV)[None, :] < p["npl"].clamp(max=T)[:, None]
    return int(((tiles * listed).sum(1) * 2 * (16 // G) < k).sum().item())


@pytest.mark.parametrize("nq,ds,distance,k", [(1300, 2, "euclidean", 100), (1024, 1, "inner", 10),
                                              (1025, 2, "inner", 128), (1024, 1, "euclidean", 1)])
def test_piece_edge_cells_ragged_probe_counts(nq, ds, distance, k):
    """probe counts drawn from 0 ... 12, and 0, 1, T - 1, T, T + 1 among them.  At most half of the queries may pass
    through the exact redo, so that the candidates carry the comparison"""
    p = _pieces_problem(50 + ds + k, nq, ds, ragged=True, long_first=k >= 100)
    assert _gate(p, k)
    few = _few_maxima(p, k)
    assert few <= nq // 2
    scan = _check(p, k, distance, expect=True)
    assert scan.last_redone(nq) <= few


def test_probe_repeated_across_the_first_pass_boundary():
    nq = 1100
    p = _pieces_problem(60, nq, 2, ragged=False, long_first=True)
    q = torch.arange(nq, device=DEV)
    p["cells"][q % 3 == 0, T] = p["cells"][q % 3 == 0, T - 1]
    p["cells"][q % 3 == 1, T - 1] = p["cells"][q % 3 == 1, T - 2]
    few = _few_maxima(p, 100)
    assert few <= nq // 2
    scan = _check(p, 100, expect=True)
    assert scan.last_redone(nq) <= few


@pytest.mark.parametrize("ds,distance,k", [(2, "euclidean", 100), (1, "inner", 10)])
def test_seeded_form_over_the_same_cells(ds, distance, k):
    """the candidates proper in the seeded form (cell_threshold=False) with the seeds' threshold, over the cells at which a
    piece begins, ends or is empty: pieces of pass B under a variant build with TPQ_CELL_PIECES_B > 1; under the product
    build (B = 1) this is the undivided kernel over those cells"""
    from torchpq_amd import kernels as K
    p = _pieces_problem(70 + ds, 1100, ds, ragged=True)
    scan = K.IVFPQTopkHip(m=64)
    cs, sz = p["start"][p["cells"]].contiguous(), p["sizes"][p["cells"]].contiguous()
    got = scan.topk_fused(p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], k,
                          distance=distance, packed=K.PackCodesHip()(p["storage"]), cells=p["cells"], n_cells=N_CELLS,
                          slots_hint=int(p["sizes"].float().mean().item() * N_PROBE), cell_threshold=False)
    torch.cuda.synchronize()
    assert scan.last_cell_major() is True and scan.last_cell_threshold() is False
    ref, _ = _search(p, k, distance, cells=False, packed=False)
    assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))
    assert torch.equal(got[1], ref[1])
