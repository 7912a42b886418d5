"""What the tests of the cell-major form's kept state share (csrc/scan_cells.hip, `The kept state`;
tpq_ivfpq_search_fused_cells_kept): the state's layout and the split codebook restated in numpy, a provider of states as
IVFPQIndex hands one to the scan, and the guarded-buffer cases of the new entry point.

The guarded cases are added to the table of tests/guarded_cases.py and to the builders of
tests/test_gpu_guarded_buffers.py from here, as tests/ivfpq4_filtered_guarded.py adds its own: importing this module
registers them (once) and needs no GPU; tests/test_scan_cell_kept_cpu.py and tests/test_gpu_scan_cell_kept.py import it,
so a run that collects the suite has them in the table before any test runs, and
tests/test_gpu_scan_cell_kept.py::test_guards_hold_and_results_do_not_depend_on_the_fill runs them.
tests/test_guarded_alloc_cpu.py run on its own, with neither of the two collected, reports the entry point as lacking a
case: the table's own file is the place for these lines, and they are here only because no existing test file is edited.
"""
import numpy as np

import guarded_cases as gc

SCALE_EXP = 12   # kCellScaleExp: the largest scaled entry lies in [2^12, 2^13)


def align(n):
    return (n + 255) // 256 * 256


def kept_bytes(n_slots, ds):
    """[256 bytes: parameters][the codebook image: 64 x 256 x 4 ds bytes][an fp32 per slot address, rounded up to 256]"""
    return 256 + 64 * 256 * 4 * ds + align(4 * n_slots)


def scale(codebook):
    """s_x: the power of two that brings the largest |entry| into [2^12, 2^13) (cell_prep_kernel)"""
    top = np.abs(codebook.astype(np.float32)).max()
    e = int((top.view(np.uint32) >> 23) & 255) - 127
    return np.float32(2.0 ** (SCALE_EXP - e))


def split_image(codebook):
    """the codebook [64][ds][256] f32 as a candidate workgroup keeps it, as uint16 [64][256][2 ds]: per entry (j, c) the
    ds hi pieces fp16(s_x c), then the ds lo pieces fp16(s_x c - hi) -- ds = 2: the dwords (h0 h1), (l0 l1); ds = 1: the
    dword (h l).  The scaling by a power of two is exact; both conversions round to nearest even."""
    ys = codebook.astype(np.float32) * scale(codebook)          # [j][e][c]
    hi = ys.astype(np.float16)
    lo = (ys - hi.astype(np.float32)).astype(np.float16)
    img = np.concatenate([hi.transpose(0, 2, 1), lo.transpose(0, 2, 1)], axis=2)   # [j][c][h.., l..]
    return np.ascontiguousarray(img).view(np.uint16)


def views(buf, n_slots, ds):
    """(parameters f32 [4], image u16 [64][256][2 ds], norms f32 [n_slots]) of a state's bytes (a numpy uint8 array)"""
    book = 64 * 256 * 4 * ds
    return (buf[:16].view(np.float32), buf[256:256 + book].view(np.uint16).reshape(64, 256, 2 * ds),
            buf[256 + book:256 + book + 4 * n_slots].view(np.float32))


class Provider:
    """what IVFPQIndex._cell_kept_state is to the scan: one state, created when first asked for"""

    def __init__(self):
        self.state, self.asked = None, 0

    def __call__(self, n_bytes, device):
        from torchpq_amd.kernels import CellKeptState
        self.asked += 1
        if self.state is None:
            self.state = CellKeptState(n_bytes, device)
        assert self.state.buf.numel() >= n_bytes
        return self.state


def run(p, k, distance="euclidean", kept=None, scan=None, cell_threshold=True):
    """test_gpu_scan_cells._search with a kept state and the switch of the two forms"""
    import torch
    from torchpq_amd import kernels as K
    scan = scan or K.IVFPQTopkHip(m=64)
    scan.keep_workspace = True
    cs, sz = p["start"][p["cells"]].contiguous(), p["sizes"][p["cells"]].contiguous()
    hint = int(p["sizes"].float().mean().item() * p["cells"].shape[1])
    pk = p.setdefault("packed", K.PackCodesHip()(p["storage"]))
    out = scan.topk_fused(p["storage"], p["query"], p["codebook"], p["is_empty"], cs, sz, p["npl"], k, distance=distance,
                          packed=pk, slots_hint=hint, cells=p["cells"], n_cells=p["n_cells"],
                          cell_threshold=cell_threshold, kept=kept)
    torch.cuda.synchronize()
    return out, scan


# ---- guarded-buffer cases ------------------------------------------------------------------------------------------
CASE_SYMBOLS = {
    "scan_cell_kept_threshold_form": ("tpq_ivfpq_search_fused_cells_kept",),
    "scan_cell_kept_seeded_form": ("tpq_ivfpq_search_fused_cells_kept",),
}


def builder(cell_threshold):
    def build():
        from test_gpu_scan_cell_threshold import _big
        p = _big(71, 1025, 12, 2, ragged=True)

        def fn():
            # a building call and a reusing call: the state and both workspaces are allocated between guards
            kept, out = Provider(), []
            for want in ("built", "reused"):
                got, scan = run(p, 10, kept=kept, cell_threshold=cell_threshold)
                assert scan.last_cell_major() is True and scan.last_cell_threshold() is cell_threshold
                assert scan.last_cell_kept == want
                out.append(got)
            return out
        return fn
    return build


def register():
    import test_gpu_guarded_buffers as gpu        # (importing it needs no GPU: its cases are built when they run)
    for cid, symbols in CASE_SYMBOLS.items():
        if cid not in gc.CASE_SYMBOLS:
            gc.CASE_SYMBOLS[cid] = symbols
            gc.CASE_IDS.append(cid)
            for s in symbols:
                gc.CASES.setdefault(s, []).append(cid)
        if cid not in gpu.BUILDERS:
            gpu.case(cid)(builder(cid.endswith("threshold_form")))


register()
