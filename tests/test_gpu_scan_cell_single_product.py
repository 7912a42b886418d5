"""GPU: the single-product selection key of the cell-major scan's threshold form (csrc/scan_cells.hip, `The
single-product key`; tpq_ivfpq_scan_use_cell_single_product; IVFPQTopkHip.last_cell_products) through
IVFPQTopkHip.topk_fused with `cells`, on the layout of tests/test_gpu_scan_cell_threshold.py: 8 or 16 cells of 512 ...
1 025 slots, 5 % tombstones, from the smallest batch the form is taken at.
  * values bit for bit and addresses entry for entry against the reference-layout kernel (`cells=False, packed=False`) and
    against the same call with the switch off; the report names the arithmetic (ds = 1 stays on three products);
  * the band: pass A read back from the kept workspace on the adversarial families of tests/scan_cells_oracle.py -- every
    surviving maximum within band / 2 of a live row's exact (float64) value, thr = M_k - band, and band / 2 at least the
    float64 model's delta1_q (tests/cell_single_product_model.py);
  * no query redone exactly -- asserted only where the float64 oracle says beforehand that every query has fewer rows
    with exact >= (k-th best - 4 delta1_q) than half its lists hold, and than the finish kernel's exact list holds."""
import numpy as np
import pytest
import torch

import cell_kept_cases as ck
import cell_single_product_model as S
import scan_cells_oracle as O
from test_gpu_scan_cell_threshold import _big, _gate
from test_gpu_scan_cells import DEV
from test_scan_cell_maxima_cpu import G, T

pytestmark = pytest.mark.gpu

CAPACITY = 1024   # entries of a query's lists (16 chunks of 64: k <= 128)


def _run(p, k, distance="euclidean", single=True, cells=True, packed=True, kept=None):
    from torchpq_amd import kernels as K
    scan = K.IVFPQTopkHip(m=64)
    scan.keep_workspace = True
    cl = p["cells"].clamp(0, p["n_cells"] - 1)
    cs, sz = p["start"][cl].contiguous(), p["sizes"][cl].contiguous()
    hint = int(p["sizes"].float().mean().item() * p["cells"].shape[1])
    pk = p.setdefault("packed", K.PackCodesHip()(p["storage"])) if packed else None
    out = scan.topk_fused(p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], k, distance=distance,
                          packed=pk, slots_hint=hint, cells=p["cells"] if cells else None, n_cells=p["n_cells"],
                          cell_single_product=single, kept=kept)
    torch.cuda.synchronize()
    return out, scan


def _equal(a, b, nan_rows=None):
    ok = torch.ones(a[0].shape[0], dtype=torch.bool, device=DEV)
    if nan_rows is not None:   # (NaN values compare unequal to themselves: those rows are checked through the addresses)
        ok[nan_rows] = False
    return torch.equal(a[0][ok].view(torch.int32), b[0][ok].view(torch.int32)) and torch.equal(a[1], b[1])


def _check(p, k, distance="euclidean", nan_rows=None, kept=None):
    """switch on against the reference-layout kernel and against switch off; -> the scan of the call with the switch on"""
    ds = p["codebook"].shape[1]
    ref, _ = _run(p, k, distance, cells=False, packed=False)
    off, scan3 = _run(p, k, distance, single=False)
    assert scan3.last_cell_threshold() is True and scan3.last_cell_products() == 3
    on, scan = _run(p, k, distance, kept=kept)
    assert scan.last_route() == "dump_sel16" and scan.last_cell_threshold() is True
    assert scan.last_cell_products() == (1 if ds == 2 else 3)
    assert _equal(on, ref, nan_rows) and _equal(off, ref, nan_rows) and _equal(on, off, nan_rows)
    return scan


def _exact(p, distance):
    """float64 [nq, n_slots] on the decoded fp32 data"""
    ds = p["codebook"].shape[1]
    cb = p["codebook"].double().cpu().numpy()
    codes = p["storage"].permute(1, 0, 2).reshape(p["n_slots"], 64).cpu().numpy().astype(np.int64)
    xhat = cb[np.arange(64)[None, :], :, codes].reshape(p["n_slots"], 64 * ds)
    q = p["query"].double().cpu().numpy().T
    if distance != "euclidean":
        return q @ xhat.T
    return 2 * q @ xhat.T - (q ** 2).sum(1)[:, None] - (xhat ** 2).sum(1)[None, :]


def _listed(p, probes=None):
    """bool [nq, n_slots]: the live slots of each query's listed probes (`probes`: of its first that many)"""
    st, size = p["start"].cpu().numpy(), p["sizes"].cpu().numpy()
    cell_of = np.full(p["n_slots"], -1)
    for c in range(p["n_cells"]):
        cell_of[st[c]:st[c] + size[c]] = c
    cells, npl = p["cells"].cpu().numpy(), p["npl"].cpu().numpy()
    if probes is not None:
        npl = np.minimum(npl, probes)
    probed = np.zeros((cells.shape[0], p["n_cells"] + 1), bool)
    for j in range(cells.shape[1]):
        rows = np.nonzero(j < npl)[0]
        probed[rows, cells[rows, j]] = True
    live = cell_of >= 0
    if p["is_empty"] is not None:
        live &= p["is_empty"].cpu().numpy() == 0
    return probed[:, cell_of] & live[None, :]


def _exact_list(k):
    """entries of the finish kernel's exact list beside the single-product key (csrc/scan_host.h,
    cell_single_finish_regs): 64 x the next power of two of ceil((k + 4 (16 + k / 8)) / 64)"""
    r = (k + 4 * (16 + k // 8) + 63) // 64
    return 64 * (1 << (r - 1).bit_length())


def _near_the_kth(p, k, distance):
    """the float64 oracle's word, before the GPU run: [nq] rows of each query's listed probes with exact >= (k-th best -
    4 delta1_q) -- every candidate that can survive the finish kernel's cut is among them"""
    ex = np.where(_listed(p), _exact(p, distance), -np.inf)
    kth = np.partition(ex, -k, axis=1)[:, -k]
    d1 = S.delta1_q(p["query"].cpu().numpy(), p["codebook"].cpu().numpy(), packed=True)
    return np.where(np.isfinite(kth), (ex >= (kth - 4 * d1)[:, None]).sum(1), CAPACITY)


def _fits_by_the_oracle(p, k, distance):
    """fewer such rows than half the capacity of a query's lists, and than the exact list of the finish kernel holds"""
    return _near_the_kth(p, k, distance).max() < min(CAPACITY // 2, _exact_list(k))


CASES = [  # nq, n_probe, ds, distance, k
    (1024, T + 1, 2, "euclidean", 100), (1024, 12, 1, "inner", 10), (1024, T + 1, 1, "euclidean", 1),
    (1024, 12, 2, "inner", 128), (1025, T + 1, 1, "inner", 128), (1025, 12, 2, "euclidean", 10),
    (1025, T + 1, 2, "inner", 100), (1025, 12, 1, "euclidean", 100), (1300, T + 1, 2, "euclidean", 1),
    (1300, 12, 1, "euclidean", 128), (1300, T + 1, 1, "inner", 10), (1300, 12, 2, "euclidean", 100),
    (1024, 12, 2, "euclidean", 128), (1025, 12, 2, "inner", 10), (1300, T + 1, 2, "inner", 1),
]


@pytest.mark.parametrize("nq,n_probe,ds,distance,k", CASES)
def test_equals_the_reference_layout_kernel_and_the_switch_off(nq, n_probe, ds, distance, k):
    """1 024 queries -- the smallest batch the form is taken at --, 1 025, and 1 300 (no multiple of 32), every query with
    all its probes.  Gaussian data: the oracle finds a handful of rows within 4 delta1_q of the k-th best, so no query
    may be redone"""
    p = _big(nq + n_probe + k, nq, n_probe, ds, k=k, ragged=False)
    assert _gate(p, k)
    assert _fits_by_the_oracle(p, k, distance), "the seed is meant to leave the lists half empty"
    scan = _check(p, k, distance)
    assert scan.last_redone(nq) == 0


@pytest.mark.parametrize("n_probe,distance,k", [(T + 1, "euclidean", 100), (12, "inner", 10), (12, "euclidean", 128)])
def test_ragged_probe_counts(n_probe, distance, k):
    """probe counts drawn from 0 ... n_probe, and 0, 1, T - 1, T, T + 1 among them; only queries whose first pass reserves
    fewer than k maxima may be redone (threshold -inf: everything is admitted)"""
    p = _big(31 + n_probe + k, 1300, n_probe, 2, k=k, ragged=True)
    assert _gate(p, k)
    scan = _check(p, k, distance)
    tiles = (p["sizes"][p["cells"]] + 31) // 32
    listed = torch.arange(n_probe, device=DEV)[None, :] < p["npl"].clamp(max=T)[:, None]
    few = ((tiles * listed).sum(1) * 2 * (16 // G) < k).sum().item()
    assert scan.last_redone(1300) <= few


def test_probe_repeated_across_the_first_pass_boundary():
    p = _big(34, 1100, 12, 2, ragged=False)
    q = torch.arange(1100, device=DEV)
    p["cells"][q % 3 == 0, T] = p["cells"][q % 3 == 0, T - 1]
    p["cells"][q % 3 == 1, T - 1] = p["cells"][q % 3 == 1, T - 2]
    scan = _check(p, 100)
    assert scan.last_redone(1100) == 0


def test_integer_data_mass_ties_at_the_kth_place():
    """every value exact in any arithmetic: the ties at the k-th place are all admitted or the query is redone"""
    p = _big(33, 1100, 12, 2, integer=True)
    _check(p, 100)
    _check(p, 10, "inner")


def test_nan_inf_queries():
    nq = 1100
    p = _big(35, nq, 12, 2, ragged=False)
    p["query"][3, 7] = float("nan")
    p["query"][:, 8] = float("inf")
    p["query"][5, 9] = 1e30       # beyond the fp16 scale's range: the exact kernel's
    p["query"][:, 10] = 0.0
    scan = _check(p, 50, nan_rows=[7, 8, 9])
    assert 4 <= scan.last_redone(nq) < 4 + nq // 10


@pytest.mark.parametrize("distance,k", [("euclidean", 100), ("inner", 10)])
def test_kept_state_built_and_reused(distance, k):
    """the piece maxima travel in the state's parameter block: the call that builds it and the calls that only read it
    return the same bits; the first 16 bytes, the image and the norms are where they were"""
    nq = 1025
    p = _big(50 + k, nq, 12, 2, k=k, ragged=False)
    assert _gate(p, k)
    ref, _ = _run(p, k, distance, cells=False, packed=False)
    plain, scan = _run(p, k, distance)
    assert scan.last_cell_products() == 1 and scan.last_cell_kept is None
    band = scan.last_cell_threshold_state()["band"].clone()
    kept = ck.Provider()
    for want in ("built", "reused", "reused"):
        got, scan = _run(p, k, distance, kept=kept)
        assert scan.last_cell_kept == want and scan.last_cell_products() == 1
        assert _equal(got, ref) and _equal(got, plain)
        assert torch.equal(scan.last_cell_threshold_state()["band"], band)     # the same maxima, the same band
    off, scan = _run(p, k, distance, single=False, kept=kept)                   # the state serves both settings
    assert scan.last_cell_kept == "reused" and scan.last_cell_products() == 3 and _equal(off, ref)
    buf = kept.state.buf.cpu().numpy()
    kparams, image, _ = ck.views(buf, p["n_slots"], 2)
    assert kparams[3] == ck.scale(p["codebook"].cpu().numpy()) and kparams[2] == 1.0
    assert image.tobytes() == ck.split_image(p["codebook"].cpu().numpy()).tobytes()
    # bytes [64, 192) of the block: the packed maxima, never below the model's pair maxima and within their rounding
    pm = (buf[64:192].view(np.uint16).astype(np.uint32) << 16).view(np.float32).astype(np.float64)
    XH, XL = S.piece_maxima(S.pieces(p["query"].cpu().numpy(), p["codebook"].cpu().numpy()))
    for got_m, X in ((pm[:32], XH), (pm[32:], XL)):
        pair = X.reshape(32, 2).max(1)
        assert (got_m >= pair).all() and (got_m <= pair * 1.0002 * (1 + 2.0 ** -7)).all()


FAMILIES = [f for f in O.FAMILIES if f != "one_subq"]      # (one_subq is one query per sub-quantizer: 64 queries)


@pytest.mark.parametrize("distance", O.METRICS)
@pytest.mark.parametrize("name", FAMILIES)
def test_band_on_the_adversarial_families(name, distance):
    """1 024 queries over 8 cells of ~660 slots with the family's codebook, queries and codes, k = 20.  From the kept
    workspace: band / 2 >= the float64 model's delta1_q (exact maxima); every maximum that survived the candidate pass is
    within band / 2 of the exact value of a live row of the query's first T probes; thr = fl(M_k) - band where all
    maxima survived (folded over |q|^2 when euclidean), and M_k - band / 2 <= the exact k-th best over all listed probes"""
    from torchpq_amd._lib import load
    nq, n_probe, k, ds = 1024, 8, 20, 2
    p = _big(60, nq, n_probe, ds, ragged=False)
    assert _gate(p, k)
    cb, q, codes = O.family(name, ds, nq, p["n_slots"], seed=2)
    p["codebook"], p["query"] = torch.from_numpy(cb).to(DEV), torch.from_numpy(q).to(DEV)
    p["storage"] = torch.from_numpy(O.storage_of(codes)).to(DEV)
    p.pop("packed", None)
    got, scan = _run(p, k, distance)
    assert scan.last_cell_threshold() is True and scan.last_cell_products() == 1
    ref, _ = _run(p, k, distance, cells=False, packed=False)
    assert _equal(got, ref)
    state = {n: t.cpu().numpy() for n, t in scan.last_cell_threshold_state().items()}
    count, maxima, survived, thr, band = (state[n] for n in ("count", "maxima", "survived", "threshold", "band"))
    d1 = S.delta1_q(q, cb)
    d1_packed = S.delta1_q(q, cb, packed=True)
    exact = _exact(p, "euclidean" if distance == "euclidean" else "inner")
    first, listed = _listed(p, T), _listed(p)
    q2 = (q.astype(np.float64) ** 2).sum(0)
    fold = load().tpq_ivfpq_cell_fold_threshold
    # a family whose values crowd within the band of the k-th best (`coherent` under the euclidean metric; the scaled
    # ones wherever the larger side alone makes B^2) overflows the lists: its queries are redone exactly, and the mark
    # of that has replaced their band.  The float64 oracle says beforehand which case this is
    fits = _fits_by_the_oracle(p, k, distance)
    if fits:
        assert scan.last_redone(nq) == 0
    checked = whole = 0
    for qi in range(nq):
        if band[qi] < 0:
            # redone exactly: pass A's maxima and thr are still there; the model's band from the packed maxima (the
            # kernel's own inputs; + 2^-9: its factors 1.0001 and 1 + 2^-10 for the fp32 evaluation) stands in, and thr is only bracketed
            delta = d1_packed[qi] * (1 + 2.0 ** -9)
        else:
            checked += 1
            delta = band[qi] / 2.0
            assert d1[qi] <= delta <= d1_packed[qi] * (1 + 2.0 ** -9), (qi, d1[qi], delta, d1_packed[qi])
        n = min(count[qi], maxima.shape[1])
        kept = maxima[qi, :n][survived[qi, :n]]
        kept = kept[~np.isnan(kept)].astype(np.float64)
        ex = np.sort(exact[qi, first[qi]])
        if len(kept):
            pos = np.clip(np.searchsorted(ex, kept), 1, len(ex) - 1)
            near = np.minimum(np.abs(ex[pos] - kept), np.abs(ex[pos - 1] - kept))
            assert (near <= delta).all(), (qi, near.max(), delta)
        all_ex = np.sort(exact[qi, listed[qi]])
        kth = all_ex[-k]
        if survived[qi, :n].all() and band[qi] > 0:
            whole += 1
            m_k = np.sort(kept)[-k]
            assert m_k - delta <= kth
            want = np.float32(np.float32(m_k) - band[qi])
            if distance == "euclidean":
                assert float(thr[qi]) == fold(float(want), float(state["qnorm"][qi]))
            else:
                assert thr[qi] == want
        t = float(thr[qi]) - (q2[qi] if distance == "euclidean" else 0.0)
        assert t + delta - 1e-5 * (abs(t) + q2[qi]) <= kth
    assert not fits or checked == nq
    print(f"{name} {distance}: checked {checked}, maxima whole {whole}, redone {scan.last_redone(nq)}, "
          f"band/2 over model {np.median(band[band > 0] / 2 / d1[band > 0]):.3f}, "
          f"candidates mean {state['candidates'][band > 0].mean():.0f} max {state['candidates'].max()}")
