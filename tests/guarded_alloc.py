"""Guarded allocations for the kernel wrappers: every output and workspace between two canaries, pre-filled.

The wrappers in torchpq_amd/kernels/ allocate their outputs and workspaces with torch.empty / torch.empty_like /
torch.zeros.  `GuardedTorch` stands in for the name `torch` as those modules see it and hands every such allocation out
as a view into a larger uint8 buffer

    [ GUARD bytes of 0xA5 | payload, pre-filled with the arena's fill byte | GUARD bytes of 0xA5 ]

so that two things the suite could not see become visible:

  * a write just before or just past an output or a workspace: `Arena.check()` finds a guard byte that is no longer
    0xA5 and names the allocation (shape, dtype, the wrapper line that made it) and the first and last corrupted byte;
  * a read of a region the call never wrote: the same call under the fills 0x00 and 0xFF (`run_guarded`) gives two
    results, and they must be the same -- 0xFF makes every uncleared counter -1, every uncleared float a NaN.

What it cannot see -- a condition, not a measurement: an overrun is noticed only if it lands within GUARD = 64 KiB of
the buffer.  A wild write further out (an index computed from garbage, say) goes unnoticed here, as it does without the
harness.  Writes INSIDE the payload at a wrong place show only as a wrong result.

The payload starts GUARD bytes into a fresh caching-allocator block, a multiple of 512 bytes from its start -- the
alignment such a block itself has -- so no kernel changes its load width because of the harness.  torch.zeros arrives
zero whatever the fill.  Calls with keyword arguments the shim does not model (memory_format, pin_memory, out, ...),
and CPU allocations on a GPU arena, go to the real torch unchanged and are counted in `Arena.passed_through`.

Nothing outside torchpq_amd.kernels sees the stand-in: `install` sets the module attribute `torch` of exactly the
modules in KERNEL_MODULES through a pytest monkeypatch, which undoes it.
"""
import contextlib
import importlib
import os
import sys

GUARD = 64 * 1024
GUARD_BYTE = 0xA5
ALIGN = 512
assert GUARD % ALIGN == 0

# the modules under torchpq_amd.kernels that import torch (tests/test_guarded_alloc_cpu.py checks the list is complete)
KERNEL_MODULES = ("_common", "scan", "coarse", "kmeans", "container", "flat")
INTERCEPTED = ("empty", "empty_like", "zeros")
MODELLED_KWARGS = ("dtype", "device")

_THIS_FILE = os.path.abspath(__file__)

# allocations whose guards a check() found intact, over the whole process (the GPU module reports it)
CHECKED = {"allocations": 0, "bytes": 0, "arenas": 0}


class GuardCorrupted(AssertionError):
    pass


class Allocation:
    """one intercepted allocation: `buffer` [GUARD + nbytes + GUARD] uint8, the payload at [GUARD, GUARD + nbytes)"""

    def __init__(self, buffer, nbytes, shape, dtype, kind, site):
        self.buffer, self.nbytes, self.shape, self.dtype, self.kind, self.site = buffer, nbytes, shape, dtype, kind, site

    @property
    def payload_offset(self):
        return GUARD

    def describe(self):
        return (f"torch.{self.kind} of shape {tuple(self.shape)} {self.dtype} ({self.nbytes} bytes) "
                f"at {self.site[0]}:{self.site[1]}")


def _call_site():
    f = sys._getframe(1)
    while f is not None and os.path.abspath(f.f_code.co_filename) == _THIS_FILE:
        f = f.f_back
    return ("?", 0) if f is None else (f.f_code.co_filename, f.f_lineno)


class Arena:
    """The guarded allocations of one run.  fill: the byte every torch.empty / empty_like payload starts with;
    device_type: "cuda" (allocations on other devices pass through) or "cpu" (the harness's own tests)."""

    def __init__(self, real_torch, fill=0x00, device_type="cuda"):
        assert 0 <= fill <= 0xFF
        self.torch, self.fill, self.device_type = real_torch, int(fill), device_type
        self.allocations = []
        self.passed_through = 0

    def allocate(self, shape, dtype, device, fill, kind):
        t = self.torch
        shape = tuple(int(s) for s in shape)
        numel = 1
        for s in shape:
            assert s >= 0, shape
            numel *= s
        nbytes = numel * t.empty(0, dtype=dtype).element_size()
        buffer = t.empty(GUARD + nbytes + GUARD, dtype=t.uint8, device=device)
        buffer.fill_(GUARD_BYTE)
        payload = buffer[GUARD:GUARD + nbytes]
        payload.fill_(fill)
        self.allocations.append(Allocation(buffer, nbytes, shape, dtype, kind, _call_site()))
        return payload.view(dtype).view(shape)

    def check(self):
        """every guard byte of every allocation still holds GUARD_BYTE, else GuardCorrupted naming the allocation and
        the first and last corrupted offsets, in bytes from the payload's start (negative: before it; >= its size:
        past it).  The comparison runs on the allocation's device; one flag per allocation comes back."""
        t = self.torch
        if not self.allocations:
            return 0
        flags = []
        for a in self.allocations:
            before, after = a.buffer[:GUARD], a.buffer[GUARD + a.nbytes:]
            flags.append(((before != GUARD_BYTE).any() | (after != GUARD_BYTE).any()).reshape(1).cpu())
        flags = t.cat(flags).tolist()
        problems = []
        for a, bad in zip(self.allocations, flags):
            if not bad:
                continue
            wrong = t.nonzero(a.buffer != GUARD_BYTE).reshape(-1).cpu()
            wrong = wrong[(wrong < GUARD) | (wrong >= GUARD + a.nbytes)] - GUARD
            first, last = int(wrong[0]), int(wrong[-1])
            where = []
            if first < 0:
                where.append(f"{-first} byte(s) before the payload")
            if last >= a.nbytes:
                where.append(f"{last - a.nbytes + 1} byte(s) past its end")
            problems.append(f"guard corrupted around {a.describe()}: {len(wrong)} byte(s), first at payload offset "
                            f"{first}, last at payload offset {last} (reaches {' and '.join(where)})")
        if problems:
            raise GuardCorrupted("\n".join(problems))
        CHECKED["allocations"] += len(self.allocations)
        CHECKED["bytes"] += sum(a.nbytes for a in self.allocations)
        CHECKED["arenas"] += 1
        return len(self.allocations)


class GuardedTorch:
    """`torch` as a kernel-wrapper module sees it: every attribute is the real module's except INTERCEPTED."""

    def __init__(self, real_torch, arena):
        object.__setattr__(self, "_real", real_torch)
        object.__setattr__(self, "_arena", arena)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def __setattr__(self, name, value):
        raise AttributeError("GuardedTorch is read-only")

    def _guarded(self, kind, shape, dtype, device, fill):
        t, arena = self._real, self._arena
        dtype = t.get_default_dtype() if dtype is None else dtype
        device = t.device("cpu") if device is None else t.device(device)
        if device.type != arena.device_type:
            return None
        return arena.allocate(shape, dtype, device, fill, kind)

    @staticmethod
    def _shape(args):
        if len(args) == 1 and isinstance(args[0], (tuple, list)):
            return tuple(args[0])
        return tuple(args)

    def _modelled(self, kwargs):
        return all(k in MODELLED_KWARGS for k in kwargs)

    def empty(self, *size, **kwargs):
        out = None
        if self._modelled(kwargs) and all(isinstance(s, int) for s in self._shape(size)):
            out = self._guarded("empty", self._shape(size), kwargs.get("dtype"), kwargs.get("device"), self._arena.fill)
        if out is None:
            self._arena.passed_through += 1
            return self._real.empty(*size, **kwargs)
        return out

    def zeros(self, *size, **kwargs):
        out = None
        if self._modelled(kwargs) and all(isinstance(s, int) for s in self._shape(size)):
            out = self._guarded("zeros", self._shape(size), kwargs.get("dtype"), kwargs.get("device"), 0x00)
        if out is None:
            self._arena.passed_through += 1
            return self._real.zeros(*size, **kwargs)
        return out

    def empty_like(self, other, **kwargs):
        """(contiguous whatever the strides of `other`: the wrappers hand contiguous tensors)"""
        out = None
        if self._modelled(kwargs):
            out = self._guarded("empty_like", other.shape, kwargs.get("dtype", other.dtype),
                                kwargs.get("device", other.device), self._arena.fill)
        if out is None:
            self._arena.passed_through += 1
            return self._real.empty_like(other, **kwargs)
        return out


def kernel_modules():
    return [importlib.import_module(f"torchpq_amd.kernels.{name}") for name in KERNEL_MODULES]


def install(monkeypatch, arena):
    """`torch` of every module in KERNEL_MODULES becomes a GuardedTorch over `arena` until `monkeypatch` undoes it"""
    shim = GuardedTorch(arena.torch, arena)
    for mod in kernel_modules():
        monkeypatch.setattr(mod, "torch", shim)
    return shim


@contextlib.contextmanager
def guarded(monkeypatch, fill, device_type="cuda"):
    """a fresh arena installed for the body alone; on leaving it: undone, the device synchronised, the guards checked
    (an exception from the body passes through unchecked)"""
    import torch
    arena = Arena(torch, fill, device_type)
    with monkeypatch.context() as mp:
        install(mp, arena)
        yield arena
    if device_type == "cuda":
        torch.cuda.synchronize()
    arena.check()


def run_guarded(fn, fills=(0x00, 0xFF), *, monkeypatch, device_type="cuda"):
    """fn() once per fill, each under a fresh arena installed for that call alone; synchronises, checks the guards,
    and returns {fill: fn's result}.  The arenas stay reachable as `run_guarded.arenas` ({fill: arena})."""
    results, run_guarded.arenas = {}, {}
    for fill in fills:
        with guarded(monkeypatch, fill, device_type) as arena:
            results[fill] = fn()
        run_guarded.arenas[fill] = arena
    return results


run_guarded.arenas = {}
