"""The guarded-buffer case of the fp16 lists' cell-major scan (tpq_ivf_flat16_cells_topk), registered from here as
tests/ivfflat_cells_guarded.py registers its own and for its reason; tests/test_gpu_ivfflat_f16_cell_major.py runs it.
Importing this module needs no GPU."""
import guarded_cases as gc

CASE_SYMBOLS = {"ivfflat_f16_cell_major": ("tpq_ivf_flat16_cells_topk", "tpq_ivf_flat16_scan_topk")}


def build():
    """the case of tests/ivfflat_cells_guarded.py on packed halves: 130 queries, a cell listed by 129 of them,
    tombstones, a NaN query and a list of 64 entries that some queries overflow -- every region in use, the redo runs"""
    import ivfflat_f16_oracle as f16
    import test_gpu_ivfflat_cell_major as t
    from torchpq_amd.kernels import IVFFlat16CellTopkHip
    case = t._case(11, 24, 130, 6)
    case["query"][5, 3] = float("nan")
    args = [t.T(f16.pack(case["vectors"]).view("int32"))] + [t.T(case[name]) for name in ("query", "cs", "sz", "npl")]
    kw = dict(is_empty=t.T(case["is_empty"]), cells=t.T(case["cells"]), n_cells=len(t.CELL_SIZES))

    def fn():
        return [*IVFFlat16CellTopkHip(first_probe=2, cand_cap=64)(*args, 100, **kw)]
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
