#!/usr/bin/env python3
"""Compare the device code of two builds of one translation unit, kernel by kernel, instruction for instruction.

    hipcc ... --save-temps -c emission.hip          (once per tree; keeps <unit>-hip-amdgcn-amd-amdhsa-gfx950.s)
    scripts/device_asm_diff.py parent.s branch.s

Kernels are matched by their demangled name with the type arguments of the template list and `void` dropped
(``observation_reg_kernel<5, 5, 0>`` == ``observation_reg_kernel<5, 5, 0, float, float>``); inside a body comments,
directives and blank lines are dropped and every mangled symbol is replaced by its key and the function's number is taken out of
local labels, so that names, the order of the kernels and the compilation-unit id may differ and nothing else.  Prints one line per kernel and exits 1 on any difference.
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def key_of(dem):
    m = re.match(r"(?:void )?([\w:]+)(?:<([^>]*)>)?\(", dem)
    if not m:
        return dem
    ints = [a.strip() for a in (m.group(2) or "").split(",") if re.fullmatch(r"\s*-?\d+\s*", a)]
    return m.group(1) + ("<" + ", ".join(ints) + ">" if ints else "")


def kernels(path):
    text = open(path).read().split("\n")
    names = [m.group(1) for line in text if (m := re.match(r"\s*\.type\s+(\S+),@function", line))]
    keys = {n: key_of(d) for n, d in demangle(names).items()}
    bodies, cur = {}, None
    for line in text:
        m = re.match(r"(\S+):\s*(;.*)?$", line)
        if m and m.group(1) in keys:
            cur = keys[m.group(1)]
            bodies[cur] = []
            continue
        if cur is None:
            continue
        if re.match(r"\s*\.Lfunc_end", line) or re.match(r"\.Lfunc_end", line):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if not s or s.startswith(".") and not s.endswith(":"):
            continue
        for n, k in keys.items():
            s = s.replace(n, k)
        s = re.sub(r"\.LBB\d+_", ".LBB_", s)                # (local labels carry the function's position in its file)
        bodies[cur].append(s)
    return bodies


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k:50s} only in {'first' if k in a else 'second'}")
            bad += 1
        elif a[k] != b[k]:
            first = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
            print(f"{k:50s} DIFFERS at instruction {first}: {len(a[k])} vs {len(b[k])} lines")
            bad += 1
        else:
            print(f"{k:50s} identical, {len(a[k])} instructions and labels")
    print(f"{len(set(a) | set(b))} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
