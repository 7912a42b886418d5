#!/usr/bin/env python
"""Refactor gate: do two revisions of the HIP sources compile to the same device code, kernel by kernel?

For each translation unit, the parent's source (taken from git) and the working tree's are compiled to gfx950 device
assembly with build.sh's flags; kernels are paired by symbol and compared as text -- instruction and label lines plus
the `.amdhsa_` block (registers, LDS, scratch, wave limits), comments stripped, local labels renumbered in order of
appearance.  Prints the kernel count per unit and every kernel that differs, is missing or is new; exit status 1 if any.

    python tools/isa_diff.py [--parent HEAD] [--jobs 8] [--cache DIR] [--explain] [unit ...]

--explain adds, for every kernel that differs, the `.amdhsa_` lines that changed, the instruction total before and after
and the count delta per mnemonic.  A kernel whose parameter types were renamed (another mangled symbol, the same name) is
paired by its demangled name (c++filt) instead of being reported as missing and new.

A unit is a file of torchpq_amd/csrc, `scan_packed.hip:64` for one per-M unit, or `old.hip=new1.hip+new2.hip` for a
unit the working tree has split: the parent's kernels of old.hip against the union of the new units'.  The left side
takes several units too (`old1.hip+old2.hip=new1.hip+new2.hip`) when kernels moved into a unit that already existed.  Default: scan.hip
and scan_packed.hip at every M of build.sh.  --cache keeps the parent's assembly, per revision, between runs (one check per step of a refactor).
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join("torchpq_amd", "csrc")


def compile_asm(csrc, unit, flags, out):
    src, _, m = unit.partition(":")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *flags, *([f"-DTPQ_PACKED_M={m}"] if m else []),
           "-x", "hip", "--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out]
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)  # (warnings are dropped; a failed compile shows them)
    if r.returncode:
        sys.exit(f"{unit}: hipcc failed ({csrc})\n{r.stderr[-4000:]}")


def kernels(path):
    """{symbol: normalised text} of every kernel of one assembly file: its body, then its .amdhsa_ block"""
    bodies, blocks, cur = {}, {}, None
    for line in open(path):
        line = line.split(";")[0].rstrip()
        head = line.split()[0] if line.strip() else ""
        if head == ".amdhsa_kernel":  # (the block follows the kernel's last instruction, ahead of its .Lfunc_end)
            cur = blocks.setdefault(line.split()[1], [])
        elif head == ".end_amdhsa_kernel" or head.startswith(".Lfunc_end"):
            cur = None
        elif cur is None:
            if head.endswith(":") and line[0] not in ". \t":
                cur = bodies.setdefault(head[:-1], [])
        elif head and (not head.startswith(".") or head.endswith(":") or head.startswith(".amdhsa_")):
            cur.append(" ".join(line.split()))  # an instruction, a label, or a line of the resource block
    out = {}
    for name, blk in blocks.items():
        labels = {}
        out[name] = re.sub(r"\.L[A-Za-z_]+\d+(?:_\d+)?", lambda t: labels.setdefault(t.group(0), f".L{len(labels)}"),
                           "\n".join(bodies[name] + blk))
    return out


def unqualified(symbols):
    """{demangled name without its parameter list: symbol}"""
    if not symbols:
        return {}
    try:
        names = subprocess.run(["c++filt", *symbols], stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    except (OSError, subprocess.CalledProcessError):  # no demangler: the kernels stay "missing" and "new"
        return {}
    return {n[:n.rindex("(")] if "(" in n else n: s for n, s in zip(names, symbols)}


def explain(old, new):
    """what changed in a kernel that differs: its resource lines, the instruction total, the count per mnemonic"""
    from collections import Counter
    split = lambda t: ({l.split()[0]: " ".join(l.split()[1:]) for l in t.split("\n") if l.startswith(".amdhsa_")},
                       Counter(l.split()[0] for l in t.split("\n") if not l.startswith(".") and not l.endswith(":")))
    (ro, co), (rn, cn) = split(old), split(new)
    out = [f"{k} {ro.get(k, '(absent)')}  ->  {rn.get(k, '(absent)')}" for k in sorted(set(ro) | set(rn)) if ro.get(k) != rn.get(k)]
    to, tn = sum(co.values()), sum(cn.values())
    out.append(f"instructions {to} -> {tn} ({100.0 * (tn - to) / to:+.2f} %)")
    delta = {k: cn[k] - co[k] for k in sorted(set(co) | set(cn)) if cn[k] != co[k]}
    out.append("per mnemonic: " + (", ".join(f"{k} {v:+d}" for k, v in delta.items()) or "equal counts (operands differ)"))
    return ["      " + l for l in out]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--explain", action="store_true", help="for every kernel that differs: the .amdhsa_ lines that "
                    "changed, the instruction count before and after, the count delta per mnemonic")
    ap.add_argument("--parent", default="HEAD")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--cache", default=None, help="directory that keeps the parent's assembly")
    ap.add_argument("units", nargs="*")
    a = ap.parse_args()
    text = open(os.path.join(ROOT, CSRC, "build.sh")).read()
    flags = re.search(r"FLAGS=\((.*?)\)", text, re.S).group(1).split()
    ms = re.search(r"for m in ([\d ]+);", text).group(1).split()
    units = a.units or ["scan.hip"] + [f"scan_packed.hip:{m}" for m in ms]
    with tempfile.TemporaryDirectory() as td:
        rev = subprocess.check_output(["git", "-C", ROOT, "rev-parse", a.parent], text=True).strip()
        old = os.path.join(a.cache or td, rev)  # (the parent's assembly, kept per revision)
        os.makedirs(old, exist_ok=True)
        subprocess.run(f"git -C '{ROOT}' archive {rev} | tar -x -C '{td}'", shell=True, check=True)
        asm = lambda u: u.replace(":", "_") + ".s"
        sides = {u: (u.split("=")[0].split("+"), u.split("=")[-1].split("+")) for u in units}  # spec -> (parent's units, ours)
        jobs = [(os.path.join(td, CSRC), o, flags, os.path.join(old, asm(o))) for olds, _ in sides.values() for o in olds
                if not os.path.exists(os.path.join(old, asm(o)))]
        jobs += [(os.path.join(ROOT, CSRC), n, flags, os.path.join(td, asm(n))) for _, ns in sides.values() for n in ns]
        with ThreadPoolExecutor(a.jobs) as ex:
            list(ex.map(lambda j: compile_asm(*j), jobs))
        bad = 0
        for u, (olds, ns) in sides.items():
            ko, kn, twice = {}, {}, []
            for side, d, us in ((ko, old, olds), (kn, td, ns)):
                for n in us:
                    kk = kernels(os.path.join(d, asm(n)))
                    twice += [f"twice {k}" for k in kk if k in side]
                    side.update(kk)
            # a kernel whose parameter TYPES were renamed has another symbol: paired by its name without the parameter list
            lost, came = unqualified([k for k in ko if k not in kn]), unqualified([k for k in kn if k not in ko])
            moved = {symbol: came[name] for name, symbol in lost.items() if name in came}
            diff = twice + [f"missing {k}" for k in ko if k not in kn and k not in moved] + \
                   [f"new {k}" for k in kn if k not in ko and k not in moved.values()]
            notes = {}
            for k in ko:
                k2 = moved.get(k, k)
                if k2 in kn and ko[k] != kn[k2]:
                    diff.append(f"differs {k}")
                    notes[diff[-1]] = explain(ko[k], kn[k2]) if a.explain else []
            print("\n  ".join([f"{u}: {len(ko)} kernels before, {len(kn)} after, {len(diff)} not identical"] +
                              [f"same name, other parameter types: {k} -> {v}" for k, v in moved.items()] +
                              [l for d in diff for l in [d] + notes.get(d, [])]))
            bad += len(diff)
    print("identical" if not bad else f"{bad} kernel(s) not identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
