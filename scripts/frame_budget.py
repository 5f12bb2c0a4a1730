"""Per-frame issue-slot budget of the barrier-paced forward kernels from a hipcc -S .s file (no GPU needed): every innermost loop of
a kernel that holds s_barrier is cut at its barriers, and the instructions of each frame are counted by class -- VALU, LDS, buffer /
global, s_waitcnt, s_nop, s_barrier, other SALU.  Prints the mean over the loop's frames and the per-frame extremes; with -v the
opcode histogram of the loop as well.  (scripts/isa_count.py counts a whole kernel body, prologue and tails included; the frame
budget needs the steady-state loop of each wave role cut at its barriers, which is what this adds.)
usage: frame_budget.py file.s kernel-name-substring [-v]"""
import re
import sys
from collections import Counter

src = open(sys.argv[1]).read()
want = sys.argv[2]
verbose = "-v" in sys.argv[3:]


def kind(op):
    if op == "s_waitcnt":
        return "waitcnt"
    if op == "s_nop":
        return "s_nop"
    if op == "s_barrier":
        return "barrier"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):          # (inline asm included: ds_write_addtid_b32 between ;;#ASMSTART / ;;#ASMEND is an LDS instruction like any other)
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "salu"
    return "other"


for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)\n\.Lfunc_end\d+:", src, re.S | re.M):
    name, body = m.group(1), m.group(2)
    if want not in name:
        continue
    print(name)
    lines = body.splitlines()
    # basic blocks with the loop the compiler's comments put them in: (loop header name or None, opcodes)
    blocks = [[None, []]]
    for line in lines:
        t = line.strip()
        b = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.\d+:)(.*)$", t)
        if b:
            rest = b.group(2)
            own = b.group(1) if "Loop Header" in rest else None
            inl = re.search(r"in Loop: Header=(BB\d+_\d+)", rest)
            blocks.append([own or (inl.group(1) if inl else None), []])
            blocks[-1].append(own is not None)
            continue
        if not t or t.startswith((".", ";")) or t.endswith(":"):
            continue
        blocks[-1][1].append(t.split()[0])
    for i, blk in enumerate(blocks):
        if len(blk) < 3 or not blk[2]:
            continue
        label = blk[0]
        # the loop in execution order: the header and the member blocks behind it, then the member blocks laid out in front of it
        j = i
        while j < len(blocks) and blocks[j][0] == label:
            j += 1
        k = i
        while k > 0 and blocks[k - 1][0] == label:
            k -= 1
        ops = [op for b in blocks[i:j] + blocks[k:i] for op in b[1]]
        if "s_barrier" not in ops:
            continue
        frames, cur = [], Counter()
        for op in ops:
            cur[kind(op)] += 1
            if op == "s_barrier":
                frames.append(cur)
                cur = Counter()
        for cls, v in cur.items():         # the loop's own bookkeeping behind the last barrier belongs to the last frame
            frames[-1][cls] += v
        n = len(frames)
        tot = Counter()
        for f in frames:
            tot.update(f)
        cols = ("valu", "lds", "vmem", "waitcnt", "s_nop", "salu", "barrier")
        print(f"  loop {label}: {n} frames, {len(ops)} instructions ({len(ops) / n:.1f} per frame)")
        print("    per frame, mean (min-max): " + "  ".join(
            f"{c} {tot[c] / n:.2f} ({min(f[c] for f in frames)}-{max(f[c] for f in frames)})" for c in cols))
        if verbose:
            hist = Counter(ops)
            print("    per frame by opcode: " + ", ".join(f"{op} {v / n:.2f}" for op, v in sorted(hist.items(), key=lambda kv: -kv[1])))
