"""The guarded-buffer cases of the four launching 4-bit range entry points (tpq_ivfpq4_range_count / _fill and their
residual forms), added to the table of tests/guarded_cases.py and to the builders of tests/test_gpu_guarded_buffers.py
from here, through that module's own `case` registration: tests/test_guarded_alloc_cpu.py asks for a guarded case for
every launching entry point that a wrapper reaches.

Importing this module registers the cases (once); both tests/test_ivfpq4_range_cpu.py and
tests/test_gpu_ivfpq4_range.py import it, so a run that collects the suite has them in the table before any test runs.
The parametrised test of tests/test_gpu_guarded_buffers.py has read the table by then, so the two cases are run by
tests/test_gpu_ivfpq4_range.py::test_guards_hold_and_results_do_not_depend_on_the_fill, on guarded_alloc.run_guarded
and that module's `same_bits`.  Importing it needs no GPU.

What this cannot give: tests/test_guarded_alloc_cpu.py run on its own, with neither new test file collected, does not
import this module and reports the four entry points as lacking a case.  The table's own file is the place for these
two lines; they are kept here only because this change adds files under tests/ and edits none.
"""
import guarded_cases as gc

CASE_SYMBOLS = {
    "ivfpq4_range": ("tpq_ivfpq4_range_count", "tpq_ivfpq4_range_fill"),
    "ivfpq4_range_residual": ("tpq_ivfpq4_range_residual_count", "tpq_ivfpq4_range_residual_fill"),
}


def builder(residual):
    def build():
        import ivfpq4_range_cases as cases
        from test_gpu_ivfpq4_range import _gpu, _run
        from torchpq_amd.kernels import IVFPQ4RangeHip
        c = cases.case(24, 2, 3, 4, "euclidean", residual)
        assert c["storage"].shape[1] % 32 != 0
        _gpu(c)
        thr = cases.thresholds(cases.candidates(c, residual, "euclidean"))

        def fn():
            op, out = IVFPQ4RangeHip(m=24), []
            for n_split in ((None,) if residual else (None, 1, 5)):
                for run, name in ((None, "median"), (0, "boundary"), (len(c["runs"]) - 1, "mixed0")):
                    out.append(_run(c, residual, thr[name], "euclidean", run=run, n_split=n_split, op=op)[:3])
                    if not residual:
                        assert op.last_n_split == n_split if n_split else op.last_n_split > 1
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
            gpu.case(cid)(builder(cid.endswith("residual")))


register()
