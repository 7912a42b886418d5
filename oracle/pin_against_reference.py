"""Pin the oracle against the reference ITSELF, executed here, or against what it returned when it last ran.

TEST INFRASTRUCTURE.  Imports DeMoriarty/TorchPQ from /root/reference through oracle/_refimport.py
(stub cupy: only the reference's own CPU / PyTorch code paths can run) and checks every oracle
function that has a runnable counterpart, on fresh random inputs -- independently of the committed
golden vectors (tests/golden/, which were produced by the same reference and travel to the GPU box).

    PYTHONDONTWRITEBYTECODE=1 python -m oracle.pin_against_reference        # prints one line per check

Every output of the reference goes through one source: `LiveReference` runs the reference and keeps what it
returned (`recorded`: tests/golden/make_golden.py stores it as fx_pin); `RecordedReference` hands back those
arrays, so that the same checks, on the same inputs (fixed seeds), run where the reference tree is not present.
tests/test_oracle_golden.py::test_oracle_pinned_against_live_reference runs the recorded pins everywhere and the
live ones where the reference tree is present.  What cannot be pinned this way -- the list scan, which has no
CPU implementation in the reference -- is pinned indirectly (identity with the reference's
precompute_adc / decode / metric, see ivfpq_oracle.py's header).
"""
from __future__ import annotations

import numpy as np

from . import ivfpq_oracle as orc
from ._refimport import available, import_reference


class LiveReference:
    """ref(key, fn): runs fn(reference module) -> tuple of arrays, keeps them under key.0, key.1, ..."""

    def __init__(self):
        assert available(), "the reference tree is not present"
        self.tq = import_reference()
        self.recorded = {}

    def __call__(self, key, fn):
        out = [np.array(x) for x in fn(self.tq)]
        for i, x in enumerate(out):
            self.recorded[f"{key}.{i}"] = x
        return out


class RecordedReference:
    """ref(key, fn): the arrays a LiveReference kept under key (fn is not run)"""

    def __init__(self, arrays):
        self.arrays = arrays

    def __call__(self, key, fn):
        out, i = [], 0
        while f"{key}.{i}" in self.arrays:
            out.append(self.arrays[f"{key}.{i}"])
            i += 1
        assert out, f"no recorded reference output {key!r}"
        return out


def _nonneg(rng, d, n):
    """non-negative data: the reference's CPU k-means paths abs() their inputs (KMeans.py:347)"""
    return np.abs(rng.standard_normal((d, n)) * 20).astype(np.float32)


def run(verbose=True, ref=None):
    """`ref`: LiveReference (default) or RecordedReference; returns the names of the checks that held"""
    ref = LiveReference() if ref is None else ref
    import torch

    def t(x):
        return torch.from_numpy(np.array(x, copy=True))

    rng = np.random.default_rng(2024)
    done = []

    def ok(name):
        done.append(name)
        if verbose:
            print("pinned:", name)

    # coarse similarities (metric.py:31-98)
    a, b = _nonneg(rng, 48, 37), _nonneg(rng, 48, 29)
    ref_s, = ref("sims", lambda tq: (tq.metric.negative_squared_l2_distance(t(a), t(b)).numpy(),))
    got = orc.neg_sq_l2(a, b)
    np.testing.assert_allclose(got, ref_s, rtol=1e-5, atol=1e-5 * np.abs(ref_s).max())
    ok("neg_sq_l2 == metric.negative_squared_l2_distance")

    # ADC look-up table (codec/PQCodec.py:62-75) on a codec with injected codebooks
    m, ds, nq = 8, 4, 19
    cb = (rng.standard_normal((m, ds, 256)) * 10).astype(np.float32)

    def codec_of(tq):
        codec = tq.codec.PQCodec(d_vector=m * ds, n_subvectors=m, n_clusters=256, distance="euclidean")
        codec.kmeans.register_buffer("centroids", t(cb))
        codec._is_trained = torch.tensor(True) if hasattr(codec, "_is_trained") else True
        return codec

    q = (rng.standard_normal((m * ds, nq)) * 10).astype(np.float32)
    ref_lut, = ref("adc_lut", lambda tq: (codec_of(tq).precompute_adc(t(q)).numpy(),))
    got = orc.adc_lut(q, cb, "euclidean")
    np.testing.assert_allclose(got, ref_lut, rtol=1e-4, atol=1e-4 * np.abs(ref_lut).max())
    ok("adc_lut == PQCodec.precompute_adc")

    # decode (codec/PQCodec.py:95-130)
    codes = rng.integers(0, 256, (m, 50), dtype=np.uint8)
    ref_dec, = ref("decode", lambda tq: (codec_of(tq).decode(t(codes)).numpy(),))
    assert np.array_equal(orc.pq_decode(cb, codes), ref_dec)
    ok("pq_decode == PQCodec.decode")

    # smart probing (index/IVFPQIndex.py:499-512), the torch expression evaluated as the reference does
    n_probe = 16
    sims = -np.sort(np.abs(rng.standard_normal((200, n_probe)).astype(np.float32)) * 3e4, axis=1)
    ts = t(sims)
    p = torch.softmax(-ts.abs().sqrt() / 30.0, dim=-1)
    ne = -torch.sum(p * torch.log2(p) / torch.log2(torch.tensor(n_probe)), dim=-1)
    ref_np = torch.ceil(ne * n_probe).long().numpy()
    got = orc.smart_probing(sims, n_probe, 30.0)
    assert np.abs(got - ref_np).max() <= 1 and (got != ref_np).mean() < 0.01
    ok("smart_probing == IVFPQIndex.search's entropy rule")

    # container: add sequences with growth, look-ups (container/CellContainer.py:97-367)
    buffers = ("_storage", "_cell_start", "_cell_size", "_cell_capacity", "_is_empty", "_address2id")
    for mode, step in (("double", 8), ("step", 8)):
        box = {}

        def container(tq):
            if "c" not in box:
                box["c"] = tq.container.CellContainer(code_size=8, n_cells=6, dtype="uint8", device="cpu",
                                                      initial_size=4, expand_step_size=step, expand_mode=mode,
                                                      use_inverse_id_mapping=True, contiguous_size=4)
            return box["c"]

        def add(tq, data, cells):
            c = container(tq)
            r_ids, r_adr = c.add(t(data), t(cells), return_address=True)
            return (r_ids.numpy(), r_adr.numpy(), c.get_ioa(t(cells)).numpy(),
                    *[getattr(c, name).numpy() for name in buffers])

        o = orc.ContainerState(8, 6, 4, expand_step_size=step, expand_mode=mode)
        for nb in (5, 23, 2, 61):
            data = rng.integers(0, 256, (8, nb), dtype=np.uint8)
            cells = rng.integers(0, 6, nb).astype(np.int64)
            r_ids, r_adr, r_ioa, *r_buf = ref(f"container_{mode}_{nb}", lambda tq: add(tq, data, cells))
            assert np.array_equal(r_ioa, orc.get_ioa(cells))
            o_ids, o_adr = o.add(data, cells)
            assert np.array_equal(r_ids, o_ids) and np.array_equal(r_adr, o_adr)
            for name, got_buf, arr in zip(buffers, r_buf, (o.storage, o.cell_start, o.cell_size, o.cell_capacity,
                                                            o.is_empty, o.address2id)):
                assert np.array_equal(got_buf, arr), (mode, nb, name)
        probe = np.arange(-2, o.cell_capacity.sum() + 2).astype(np.int64)

        def look_ups(tq):
            c = container(tq)
            assert c.capacity + 4 == probe.shape[0]
            return (c.get_cell_by_address(t(probe)).numpy(), c.get_id_by_address(t(probe)).numpy(),
                    c.get_data_by_address(t(probe)).numpy())

        r_cell, r_id, r_data = ref(f"container_{mode}_look_ups", look_ups)
        assert np.array_equal(r_cell, orc.get_cell_by_address(probe, o.cell_start, o.cell_capacity))
        assert np.array_equal(r_id, orc.get_id_by_address(o.address2id, probe))
        assert np.array_equal(r_data, orc.storage_to_codes(o.storage, probe))
    ok("ContainerState.add / expand / get_ioa / look-ups == CellContainer (double and step)")

    # k-means assign / update (clustering/MultiKMeans.py:334-392, CPU paths; last point unlabelled)
    l, d, n, k = 3, 6, 700, 16
    data = np.stack([_nonneg(rng, d, n) for _ in range(l)])
    init = data[:, :, rng.choice(n, k, replace=False)].copy()
    full = orc.max_sim(data, init, "euclidean", "expanded")[1]

    def kmeans(tq):
        mk = tq.clustering.MultiKMeans(n_clusters=k, distance="euclidean", max_iter=1)
        _, lab = mk.get_labels(t(data), t(init))
        return (lab.numpy(), mk.euc_sim(t(data), t(init)).numpy(), mk.compute_centroids(t(data), t(full)).numpy())

    ref_lab, sims, ref_c = ref("kmeans", kmeans)
    ref_lab = ref_lab[:, :-1]
    gap = np.sort(sims, -1)[..., -1] - np.sort(sims, -1)[..., -2]
    got_lab = full[:, :-1]
    same = got_lab == ref_lab
    # disagreements only where the two best centroids are (nearly) tied
    assert same.mean() > 0.99, same.mean()
    assert np.all(gap[:, :-1][~same] <= 1e-3 * np.abs(sims).max()), gap[:, :-1][~same]
    np.testing.assert_allclose(orc.compute_centroids(data, full, k), ref_c, rtol=1e-5, atol=1e-4)
    ok("max_sim / compute_centroids == MultiKMeans.get_labels / compute_centroids")

    # residual tables (index/IVFPQIndex.py:160-170, 366-405) on a CPU-trained residual index
    base = _nonneg(rng, 16, 1200)
    xq = _nonneg(rng, 16, 9)

    def residual(tq):
        np.random.seed(7)
        idx = tq.index.IVFPQIndex(d_vector=16, n_subvectors=4, n_cells=8, initial_size=256, device="cpu",
                                  pq_use_residual=True)
        idx.train(t(base))
        p1, p2 = idx.precomputed_adc_residual_precomputed(t(xq))
        return (idx.vq_codec.codebook.numpy(), idx.pq_codec.codebook.numpy(), np.ascontiguousarray(p1.numpy()),
                np.ascontiguousarray(p2.numpy()))

    vq_cb, pq_cb, p1, p2 = ref("residual", residual)
    np.testing.assert_allclose(orc.residual_part1(xq, pq_cb), p1, rtol=1e-4, atol=1e-4 * np.abs(p1).max())
    np.testing.assert_allclose(orc.residual_part2(vq_cb, pq_cb), p2, rtol=1e-4, atol=1e-4 * np.abs(p2).max())
    ok("residual_part1 / residual_part2 == IVFPQIndex.precomputed_adc_residual_precomputed")
    return done


if __name__ == "__main__":
    run()
