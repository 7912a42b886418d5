"""The guarded-allocation harness (tests/guarded_alloc.py) on CPU tensors, and the two completeness checks that keep it
honest: every allocator call in torchpq_amd/kernels/ is intercepted or allow-listed with a reason, and every library
entry point with a workspace, or reached by a wrapper, has a guarded case (tests/guarded_cases.py).  No GPU."""
import ast
import glob
import os

import pytest
import torch

import guarded_alloc as ga
import guarded_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_FILES = sorted(glob.glob(os.path.join(ROOT, "torchpq_amd", "kernels", "*.py")))


@pytest.fixture
def arena():
    return ga.Arena(torch, fill=0xFF, device_type="cpu")


# ---- the harness itself ---------------------------------------------------------------------------------------------
def test_alloc_pair_under_the_proxy_is_a_view_of_a_guarded_buffer(monkeypatch, arena):
    from torchpq_amd.kernels import _common
    ga.install(monkeypatch, arena)
    v, a = _common.alloc_pair(5, 7, "cpu")
    assert v.shape == (5, 7) and v.dtype == torch.float32 and a.shape == (5, 7) and a.dtype == torch.int64
    assert v.is_contiguous() and a.is_contiguous() and len(arena.allocations) == 2
    for t, alloc in zip((v, a), arena.allocations):
        assert t.data_ptr() == alloc.buffer.data_ptr() + ga.GUARD
        assert alloc.buffer.numel() == 2 * ga.GUARD + t.numel() * t.element_size()
        assert alloc.site[0].endswith(os.path.join("kernels", "_common.py"))
    assert arena.check() == 2
    monkeypatch.undo()
    assert _common.torch is torch


@pytest.mark.parametrize("where", ["before", "after"])
def test_a_one_byte_write_next_to_the_payload_is_reported(arena, where):
    gt = ga.GuardedTorch(torch, arena)
    gt.empty(3, 5, dtype=torch.int32, device="cpu")
    second, line = gt.empty((11,), dtype=torch.float32, device="cpu"), _here()
    gt.zeros(4, dtype=torch.uint8, device="cpu")
    assert arena.check() == 3
    alloc = arena.allocations[1]
    offset = -1 if where == "before" else second.numel() * 4
    alloc.buffer[ga.GUARD + offset] = 0
    with pytest.raises(ga.GuardCorrupted) as err:
        arena.check()
    msg = str(err.value)
    assert "(11,)" in msg and "torch.float32" in msg and f"{os.path.basename(__file__)}:{line}" in msg
    assert f"first at payload offset {offset}, last at payload offset {offset}" in msg
    assert ("1 byte(s) before the payload" if where == "before" else "1 byte(s) past its end") in msg
    assert "(3, 5)" not in msg and "(4,)" not in msg          # the neighbours are not blamed


def _here():
    import sys
    return sys._getframe(1).f_lineno


def test_first_and_last_corrupted_offsets(arena):
    gt = ga.GuardedTorch(torch, arena)
    t = gt.empty(10, dtype=torch.int64, device="cpu")
    buf = arena.allocations[0].buffer
    buf[ga.GUARD + 80 + 3] = 1
    buf[ga.GUARD + 80 + 4000] = 0x5A
    with pytest.raises(ga.GuardCorrupted, match="2 byte.s., first at payload offset 83, last at payload offset 4080"):
        arena.check()
    buf[ga.GUARD + 80 + 4000] = ga.GUARD_BYTE
    buf[ga.GUARD + 80 + 3] = ga.GUARD_BYTE
    assert arena.check() == 1 and t.numel() == 10


def test_a_write_inside_the_payload_leaves_the_guards_alone(arena):
    gt = ga.GuardedTorch(torch, arena)
    t = gt.empty(6, 2, dtype=torch.float32, device="cpu")
    t.fill_(3.0)
    t[-1, -1] = 7.0
    t[0, 0] = 9.0
    assert arena.check() == 1


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x3C])
def test_every_fill_arrives_and_zeros_is_zero(fill):
    arena = ga.Arena(torch, fill=fill, device_type="cpu")
    gt = ga.GuardedTorch(torch, arena)
    e = gt.empty(7, 3, dtype=torch.int32, device="cpu")
    like = gt.empty_like(torch.zeros(5, 2, dtype=torch.int64))
    z = gt.zeros(9, dtype=torch.float32, device="cpu")
    assert (e.view(torch.uint8) == fill).all() and (like.view(torch.uint8) == fill).all()
    assert like.shape == (5, 2) and like.dtype == torch.int64
    assert (z.view(torch.uint8) == 0).all() and z.dtype == torch.float32
    if fill == 0xFF:
        assert (e == -1).all()
    assert arena.check() == 3 and arena.passed_through == 0


def test_shapes_as_ints_as_a_tuple_and_empty(arena):
    gt = ga.GuardedTorch(torch, arena)
    a = gt.empty(2, 3, 4, dtype=torch.uint8, device="cpu")
    b = gt.empty((2, 3, 4), dtype=torch.uint8, device="cpu")
    c = gt.empty(torch.Size([2, 3]), dtype=torch.float32, device=torch.device("cpu"))
    d = gt.empty(0, dtype=torch.int64, device="cpu")
    e = gt.empty(0, 5, dtype=torch.float32, device="cpu")
    f = gt.zeros((0,), dtype=torch.int32, device="cpu")
    g = gt.empty(0, device="cpu")                                   # (kernels/kmeans.py: no dtype -> the default)
    h = gt.empty_like(torch.zeros(0, 3, dtype=torch.uint8))
    assert a.shape == b.shape == (2, 3, 4) and c.shape == (2, 3) and c.dtype == torch.float32
    assert d.shape == (0,) and e.shape == (0, 5) and f.shape == (0,) and h.shape == (0, 3)
    assert d.dtype == torch.int64 and g.dtype == torch.get_default_dtype() and f.dtype == torch.int32
    assert arena.check() == 8 and arena.passed_through == 0
    # the two guards of an empty allocation meet: a byte at the payload's place is a corrupted guard
    arena.allocations[3].buffer[ga.GUARD] = 0
    with pytest.raises(ga.GuardCorrupted, match="last at payload offset 0 .reaches 1 byte.s. past its end"):
        arena.check()


def test_the_payload_offset_is_a_multiple_of_512(arena):
    gt = ga.GuardedTorch(torch, arena)
    for shape, dtype in (((1,), torch.uint8), ((3, 5), torch.float32), ((1001,), torch.int64), ((0,), torch.int32)):
        t = gt.empty(*shape, dtype=dtype, device="cpu")
        alloc = arena.allocations[-1]
        assert alloc.payload_offset % 512 == 0 and alloc.payload_offset == ga.GUARD == 64 * 1024
        if t.numel():       # (a tensor without elements reports a null address, guarded or not)
            assert t.data_ptr() - alloc.buffer.data_ptr() == alloc.payload_offset
            assert t.data_ptr() % t.element_size() == 0
        else:
            assert t.storage_offset() * t.element_size() == alloc.payload_offset


def test_unsupported_keywords_and_other_devices_pass_through(arena):
    gt = ga.GuardedTorch(torch, arena)
    a = gt.empty(3, 4, dtype=torch.float32, device="cpu", memory_format=torch.contiguous_format)
    b = gt.zeros(5, dtype=torch.int32, device="cpu", pin_memory=False)
    out = torch.ones(6)
    c = gt.zeros(6, out=out)
    d = gt.empty_like(torch.zeros(2, 2), memory_format=torch.preserve_format)
    assert a.shape == (3, 4) and (b == 0).all() and c is out and (out == 0).all() and d.shape == (2, 2)
    assert arena.passed_through == 4 and not arena.allocations
    gpu_arena = ga.Arena(torch, fill=0xFF, device_type="cuda")
    gg = ga.GuardedTorch(torch, gpu_arena)
    e = gg.empty(3, dtype=torch.float32, device="cpu")              # a CPU allocation on a GPU arena
    f = gg.empty(3)                                                 # ... no device at all is the CPU too
    assert e.device.type == f.device.type == "cpu"
    assert gpu_arena.passed_through == 2 and not gpu_arena.allocations


def test_everything_else_is_the_real_module(arena):
    gt = ga.GuardedTorch(torch, arena)
    assert gt.float32 is torch.float32 and gt.cuda is torch.cuda and gt.is_tensor(torch.zeros(1))
    assert gt.full((2,), 3.0).tolist() == [3.0, 3.0] and gt.arange(3).tolist() == [0, 1, 2]
    with pytest.raises(AttributeError):
        gt.empty = None
    assert not arena.allocations


def test_run_guarded_installs_per_fill_and_undoes(monkeypatch):
    from torchpq_amd.kernels import _common, scan
    seen = []

    def fn():
        seen.append((_common.torch._arena.fill, scan.torch is _common.torch))
        return _common.alloc_pair(2, 2, "cpu")[1].clone()

    out = ga.run_guarded(fn, monkeypatch=monkeypatch, device_type="cpu")
    assert seen == [(0x00, True), (0xFF, True)]
    assert (out[0x00] == 0).all() and (out[0xFF] == -1).all()
    assert all(mod.torch is torch for mod in ga.kernel_modules())

    def overrun():
        t = _common.alloc_pair(2, 2, "cpu")[0]
        _common.torch._arena.allocations[-2].buffer[ga.GUARD + 16] = 0
        return t

    with pytest.raises(ga.GuardCorrupted, match="1 byte.s. past its end"):
        ga.run_guarded(overrun, fills=(0x00,), monkeypatch=monkeypatch, device_type="cpu")
    assert all(mod.torch is torch for mod in ga.kernel_modules())


# ---- completeness of the interception ------------------------------------------------------------------------------
# torch.<allocator> calls of the wrappers that are NOT intercepted: (file, name) -> why that is right
ALLOWED = {
    ("scan.py", "full"): "the per-query threshold of a range search from a Python float: an INPUT the kernels only read",
    ("flat.py", "full"): "the per-query threshold of FlatRangeHip from a Python float: an INPUT the kernels only read",
    ("scan.py", "full_like"): "CellCandidatesHip decodes the kernel's images with torch ops after the call: no kernel "
                              "writes or reads these tensors",
}
ALLOCATOR_PREFIXES = ("empty", "zeros", "ones", "full", "new_")


def _is_allocator(name):
    return name.startswith(ALLOCATOR_PREFIXES) or name == "tensor"


def _torch_allocator_calls(path):
    tree = ast.parse(open(path).read(), path)
    for node in ast.walk(tree):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and _is_allocator(node.func.attr):
            base = node.func.value
            if isinstance(base, ast.Name) and base.id == "torch":
                yield node.func.attr, node.lineno
            elif node.func.attr.startswith("new_"):          # tensor.new_empty(...) and its kin escape the shim too
                yield node.func.attr, node.lineno


def test_every_allocator_call_of_the_wrappers_is_intercepted_or_allow_listed():
    assert len(KERNEL_FILES) >= 7
    seen, used = set(), set()
    for path in KERNEL_FILES:
        for name, line in _torch_allocator_calls(path):
            key = (os.path.basename(path), name)
            seen.add(name)
            if name in ga.INTERCEPTED:
                continue
            assert key in ALLOWED, f"{path}:{line}: torch.{name} is neither intercepted by GuardedTorch nor allow-listed"
            used.add(key)
    assert set(ga.INTERCEPTED) <= seen, "GuardedTorch intercepts an allocator the wrappers no longer use"
    assert used == set(ALLOWED), f"stale allow-list entries: {set(ALLOWED) - used}"
    assert all(len(reason) > 20 for reason in ALLOWED.values())
    for name in ga.INTERCEPTED:
        assert callable(getattr(ga.GuardedTorch, name))


def test_the_allocator_walk_sees_what_it_should(tmp_path):
    src = tmp_path / "x.py"
    src.write_text("import torch\na = torch.empty_strided((2,), (1,))\nb = a.new_zeros(3)\nc = torch.tensor([1])\n"
                   "d = torch.ones(2)\ne = torch.cat([a, a])\nf = torch.zeros_like(a)\n")
    assert sorted(n for n, _ in _torch_allocator_calls(str(src))) == ["empty_strided", "new_zeros", "ones", "tensor",
                                                                      "zeros_like"]


def test_the_shim_is_installed_in_every_kernel_module_that_imports_torch():
    importing = set()
    for path in KERNEL_FILES:
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Import) and any(a.name == "torch" and a.asname is None for a in node.names):
                importing.add(os.path.basename(path)[:-3])
            assert not (isinstance(node, ast.ImportFrom) and node.module == "torch"), \
                f"{path}: `from torch import ...` binds an allocator the shim cannot replace"
    assert importing == set(ga.KERNEL_MODULES)


# ---- completeness of the coverage ----------------------------------------------------------------------------------
SIZE_SUFFIXES = ("_workspace_bytes", "_prepared_bytes")


def _launching(name, signatures):
    """an entry point that launches: returns int and takes pointers (the size, route and `supported` queries do not)"""
    from torchpq_amd import _lib
    res, args = signatures[name]
    return res is _lib._i and _lib._vp in args and not name.startswith("tpq_ubench")


def _symbols_with_a_size_sibling():
    """every launching symbol of the signature table that shares its stem with a *_workspace_bytes / *_prepared_bytes
    function: `<stem>` itself or `<stem>_<more>` (tpq_lloyd_prepared_bytes -> tpq_lloyd_prepare by the `<stem>_prepare`
    rule)"""
    from torchpq_amd import _lib
    out = {}
    for size_fn in _lib.SIGNATURES:
        for suffix in SIZE_SUFFIXES:
            if not size_fn.endswith(suffix):
                continue
            stem = size_fn[:-len(suffix)]
            for name in _lib.SIGNATURES:
                if name.endswith(SIZE_SUFFIXES) or not _launching(name, _lib.SIGNATURES):
                    continue
                if suffix == "_prepared_bytes":
                    if name == stem + "_prepare":
                        out.setdefault(name, size_fn)
                elif name == stem or name.startswith(stem + "_"):
                    out.setdefault(name, size_fn)
    return out


def _symbols_the_wrappers_reach():
    """string literals tpq_* handed to call(...), to getattr(<lib>, ...) or to self._scan(...) / self._cell_query(...)
    in the wrappers, that name a launching entry point"""
    from torchpq_amd import _lib
    found = {}
    for path in KERNEL_FILES:
        tree = ast.parse(open(path).read(), path)
        for node in ast.walk(tree):
            if not isinstance(node, ast.Call):
                continue
            fn = node.func
            fname = fn.id if isinstance(fn, ast.Name) else fn.attr if isinstance(fn, ast.Attribute) else None
            if fname not in ("call", "getattr", "_scan"):
                continue
            for lit in ast.walk(node):
                if isinstance(lit, ast.Constant) and isinstance(lit.value, str) and lit.value.startswith("tpq_"):
                    assert lit.value in _lib.SIGNATURES, f"{path}:{lit.lineno}: {lit.value} is not in the signature table"
                    if _launching(lit.value, _lib.SIGNATURES):
                        found.setdefault(lit.value, f"{os.path.basename(path)}:{lit.lineno}")
    return found


def test_every_entry_point_with_a_workspace_has_a_guarded_case():
    from torchpq_amd import _lib
    need = _symbols_with_a_size_sibling()
    size_fns = [s for s in _lib.SIGNATURES if s.endswith(SIZE_SUFFIXES)]
    assert len(size_fns) >= 15
    assert {"tpq_ivfpq_scan_topk", "tpq_ivfpq_scan_topk_packed_tickets", "tpq_ivfpq_cell_candidates", "tpq_lloyd_prepare",
            "tpq_lloyd_step", "tpq_ivfpq_coarse_probe_prepare", "tpq_ivfpq_coarse_probe_route", "tpq_coarse_assign_route",
            "tpq_get_ioa", "tpq_flat_topk", "tpq_ivfpq4_scan_residual_topk", "tpq_ivfpq_scan_filtered_topk",
            "tpq_max_sim_select", "tpq_compute_centroids", "tpq_ivfflat_scan_topk"} <= set(need)
    # the three entry points that take a workspace sized by a function of another stem (the fused search)
    need.update({s: "tpq_ivfpq_scan_workspace_bytes" for s in _lib.SIGNATURES if s.startswith("tpq_ivfpq_search_fused")})
    missing = {s: f for s, f in need.items() if s not in guarded_cases.CASES}
    assert not missing, f"entry points with a workspace (sized by ...) and no guarded case: {missing}"


def test_every_entry_point_a_wrapper_reaches_has_a_guarded_case():
    reached = _symbols_the_wrappers_reach()
    assert len(reached) >= 45 and "tpq_ivfpq_search_fused_cells" in reached and "tpq_max_sim_split" in reached
    assert "tpq_ivfpq_range_residual_fill" in reached and "tpq_grow_cells" in reached
    missing = {s: where for s, where in reached.items() if s not in guarded_cases.CASES}
    assert not missing, f"entry points a wrapper calls (at ...) and no guarded case: {missing}"


def test_the_case_table_is_well_formed():
    from torchpq_amd import _lib
    ids = [cid for cases in guarded_cases.CASES.values() for cid in cases]
    assert all(isinstance(cid, str) and cid for cid in ids)
    for symbol, cases in guarded_cases.CASES.items():
        assert symbol in _lib.SIGNATURES, symbol
        assert len(cases) >= 1, f"{symbol}: a key without a case covers nothing"
    assert set(ids) == set(guarded_cases.CASE_IDS)
    import test_gpu_guarded_buffers as gpu        # (importing it needs no GPU: its cases are built when they run)
    assert set(gpu.BUILDERS) == set(guarded_cases.CASE_IDS), "a case in the table that the GPU module does not run, or the reverse"
    for cid, exempt in guarded_cases.NOT_BIT_EXACT.items():
        assert cid in guarded_cases.CASE_IDS and exempt["source"] and exempt["comparison"]
        module, name = exempt["comparison"].split(".")
        assert callable(getattr(__import__(module), name)), "the comparison is the existing test's own, imported"
        assert exempt["comparison"] in (gpu.__doc__ or ""), "every exemption is listed in the GPU module's docstring"
