"""The guarded-buffer case of the three filtered exact-search entry points (tpq_flat_topk_filtered,
tpq_flat_range_filtered_count / _fill), added to the table of tests/guarded_cases.py and to the builders of
tests/test_gpu_guarded_buffers.py from here, as tests/ivfpq4_range_guarded.py does and for its reason:
tests/test_guarded_alloc_cpu.py asks for a guarded case for every launching entry point a wrapper reaches, and this
change edits no file under tests/.  Both new test files import this module; the case itself is run by
tests/test_gpu_flat_filtered.py::test_filtered_search_inside_guarded_buffers.  Importing it needs no GPU."""
import guarded_cases as gc

CASE_SYMBOLS = {"flat_filtered": ("tpq_flat_topk_filtered", "tpq_flat_range_filtered_count",
                                  "tpq_flat_range_filtered_fill")}


def build():
    """three rows -- a part without an allowed slot between two that have some, the boundaries, one slot -- and a
    query whose row allows nothing, seven parts: lists and counters that only the pads / zeros path writes"""
    import test_gpu_flat_filtered as t
    from torchpq_amd.kernels import FlatRangeFilteredHip, FlatTopkFilteredHip
    y, x, a2id, masks, rows, _ = t._problem(t.CASES[3])
    args = (t.T(y), t.T(x))
    kw = dict(bits=t.T(t._pack(masks, y.shape[1])), rows=t.T(rows), address2id=t.T(a2id), n_parts=7)

    def fn():
        return [*FlatTopkFilteredHip()(*args, 100, **kw), *FlatRangeFilteredHip()(*args, -60.0, **kw)]
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
