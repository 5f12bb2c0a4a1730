#!/usr/bin/env python3
"""profiles/obs_half_resources.txt: registers, scratch and LDS of the float16 instantiations of the emission builders
(emission_half.hip) beside their float32 siblings (emission.hip), from the compiler's kernel-resource-usage remarks -- what
scripts/kernel_resources.sh prints, regrouped so that the four storage combinations of one kernel share a line.  No GPU needed.
    python scripts/obs_half_resources.py > profiles/obs_half_resources.txt"""
import os
import re
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "viterbi_spl_amd", "csrc")
KERNELS = ("observation_kernel", "observation_reg_kernel", "snippets_append_kernel")


def remarks(unit):
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
           "-fno-honor-nans", "-I../../include", "-c", "-o", "/dev/null", unit, "-Rpass-analysis=kernel-resource-usage"]
    err = subprocess.run(cmd, cwd=CSRC, capture_output=True, text=True).stderr
    res, cur = [], None
    for line in err.split("\n"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        t = m.group(1).strip()
        if t.startswith("Function Name"):
            cur = {"name": t.split(": ")[1]}
            res.append(cur)
        else:
            k, _, v = t.partition(":")
            cur[k.strip().split(" [")[0]] = v.strip()
    return res


def main():
    allr = remarks("emission.hip") + remarks("emission_half.hip")
    dem = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in allr), capture_output=True, text=True).stdout.split("\n")
    tab = {}
    for r, d in zip(allr, dem):
        m = re.match(r"(?:void )?vit::(\w+)<([^>]*)>\(", d)
        if not m or m.group(1) not in KERNELS:
            continue
        args = [a.strip() for a in m.group(2).split(",")]
        ints = tuple(int(a) for a in args if re.fullmatch(r"-?\d+", a))
        types = ["f16" if "half" in a else "f32" for a in args if not re.fullmatch(r"-?\d+", a)]
        tab.setdefault((m.group(1), ints), {})["->".join(types)] = r
    print("# Registers, scratch and LDS of the emission builders and the snippet hand-off kernel: the float16 instantiations of")
    print("# emission_half.hip beside their float32 siblings of emission.hip (both compile obs_kernels.inc).  From the compiler's")
    print("# kernel-resource-usage remarks (scripts/obs_half_resources.py), gfx950, the Makefile's flags.")
    print("# Per storage combination (logits->emissions; the snippet kernel: its input type):")
    print("#   VGPRs / SGPRs / scratch bytes per lane / occupancy in waves per SIMD.")
    print("# LDS: static bytes per block (the LDS form's rows are dynamic LDS sized at the launch: the same for every combination).")
    print("# observation_reg_kernel<NPL, SPW, MODE>, observation_kernel<EPL, MODE>.")
    print()
    combos = ["f32->f32", "f32->f16", "f16->f32", "f16->f16"]
    print(f"{'kernel':40s}" + "".join(f"{c:>22s}" for c in combos) + "   LDS")
    scratch, more = [], []
    for key in sorted(tab):
        name = f"{key[0]}<{', '.join(map(str, key[1]))}>" if key[1] else key[0]
        cs = combos if key[0] != "snippets_append_kernel" else ["f32", "f16"]
        cells = []
        for c in cs:
            r = tab[key][c]
            cells.append(f"{r['VGPRs']:>4s} /{r['TotalSGPRs']:>4s} /{r['ScratchSize']:>2s} /{r['Occupancy']:>2s}")
            if int(r["ScratchSize"]) > 0:
                scratch.append((name, c))
            if int(r["Occupancy"]) < int(tab[key][cs[0]]["Occupancy"]):
                more.append((name, c))
        lds = sorted({tab[key][c]["LDS Size"] for c in cs})
        print(f"{name:40s}" + "".join(f"{x:>22s}" for x in cells) + " " * (22 * (4 - len(cs))) + "   " + "/".join(lds))
    print()
    print(f"instantiations with scratch: {len(scratch)} {scratch if scratch else ''}".rstrip())
    print(f"instantiations with a lower occupancy than their float32 sibling: {len(more)} {more if more else ''}".rstrip())


if __name__ == "__main__":
    main()
