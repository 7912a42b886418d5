"""The guarded-buffer case of the cell-major IVFFlat scan (tpq_ivf_flat_cells_topk), added to the table of
tests/guarded_cases.py and to the builders of tests/test_gpu_guarded_buffers.py from here, as
tests/flat_filtered_guarded.py does and for its reason: tests/test_guarded_alloc_cpu.py asks for a guarded case for every
launching entry point with a workspace, and this change edits no file under tests/.  tests/test_gpu_ivfflat_cell_major.py
imports this module and runs the case (test_cell_major_inside_guarded_buffers).  Importing it needs no GPU."""
import guarded_cases as gc

CASE_SYMBOLS = {"ivfflat_cell_major": ("tpq_ivf_flat_cells_topk", "tpq_ivfflat_scan_topk")}


def build():
    """130 queries, a cell listed by 129 of them, tombstones, a NaN query (flagged by the seed kernel) and a candidate
    list of 64 entries that some queries overflow: every region of the workspace is in use, and the redo runs"""
    import test_gpu_ivfflat_cell_major as t
    from torchpq_amd.kernels import IVFFlatCellTopkHip
    case = t._case(11, 24, 130, 6)
    case["query"][5, 3] = float("nan")
    args = [t.T(case[name]) for name in ("vectors", "query", "cs", "sz", "npl")]
    kw = dict(is_empty=t.T(case["is_empty"]), cells=t.T(case["cells"]), n_cells=len(t.CELL_SIZES))

    def fn():
        return [*IVFFlatCellTopkHip(first_probe=2, cand_cap=64)(*args, 100, **kw)]
    return fn


def register():
    import test_gpu_guarded_buffers as gpu        # (importing it needs no GPU: its cases are built when they run)
    for cid, symbols in CASE_SYMBOLS.items():
        if cid not in gc.CASE_SYMBOLS:
            gc.CASE_SYMBOLS[cid] = symbols
            gc.CASE_IDS.append(cid)
            for s in symbols:
                gc.CASES.setdefault(s, []).append(cid)
        if cid not in gpu.BUILDERS:
            gpu.case(cid)(build)


register()
