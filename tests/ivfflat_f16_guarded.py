"""The guarded-buffer case of the fp16 list scan and range search, registered from here as tests/ivfflat_cells_guarded.py
registers its own and for its reason; tests/test_gpu_ivfflat_f16.py runs it.  Importing this module needs no GPU."""
import guarded_cases as gc

CASE_SYMBOLS = {"ivfflat_f16": ("tpq_ivf_flat16_scan_topk", "tpq_ivf_flat16_range_count", "tpq_ivf_flat16_range_fill")}


def build():
    """d = 17 (an odd tail), tombstones, three workgroups per query: workspace, counts, offsets and outputs in use"""
    import test_gpu_ivfflat_f16 as t
    from torchpq_amd.kernels import IVFFlat16RangeHip, IVFFlat16TopkHip
    case = t._case(17, "some", True)
    args = [t.T(case[name]) for name in ("words", "query", "cs", "sz", "npl")]
    kw = dict(is_empty=t.T(case["is_empty"]), n_split=3)

    def fn():
        return [*IVFFlat16TopkHip()(*args, 100, **kw), *IVFFlat16RangeHip()(*args, -20.0, **kw)]
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
