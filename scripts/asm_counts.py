"""Instruction counts of one kernel in hipcc -S output (gfx950), per basic block and in total, split into vector / scalar / LDS /
global memory / wait-state no-ops:  python scripts/asm_counts.py <file.s> <mangled-name substring> [--blocks] [--range <label> <label>]
Used for profiles/group_lean_resources.txt: the regions of k_bucket_groups (load rows, networks, member loop) are runs of blocks."""
import collections
import re
import sys


def kind(op):
    if op == "s_nop":
        return "nop"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def main():
    path, sub = sys.argv[1], sys.argv[2]
    per_block = "--blocks" in sys.argv
    inside = False
    blocks = []          # (label, Counter of kinds, Counter of opcodes)
    for line in open(path):
        s = line.strip()
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", s)
        if m:
            label = m.group(1)
            if not label.startswith(".L"):
                inside = sub in label
                if inside:
                    blocks.append((label, collections.Counter(), collections.Counter()))
                continue
            if inside:
                blocks.append((label, collections.Counter(), collections.Counter()))
            continue
        if not inside or not s or s.startswith((";", ".", "//")):
            continue
        if s.startswith("s_endpgm"):
            blocks[-1][1]["salu"] += 1
            continue
        op = s.split()[0]
        blocks[-1][1][kind(op)] += 1
        blocks[-1][2][op.replace("_e32", "").replace("_e64", "")] += 1
    if "--range" in sys.argv:          # --range <first label> <label behind the last>: only the blocks of one region
        first, behind = sys.argv[sys.argv.index("--range") + 1:][:2]
        labels = [b[0] for b in blocks]
        blocks = blocks[labels.index(first):labels.index(behind) if behind in labels else len(blocks)]
    tot, ops = collections.Counter(), collections.Counter()
    for label, k, o in blocks:
        tot.update(k)
        ops.update(o)
        if per_block and sum(k.values()):
            dpp = sum(n for name, n in o.items() if name.endswith("_dpp"))
            print("%-12s %5d  valu %4d (dpp %3d, min/max %3d, cndmask %3d, readlane %2d)  salu %4d  lds %3d  vmem %2d  nop %3d" % (
                label, sum(k.values()), k["valu"], dpp, sum(n for name, n in o.items() if name.startswith(("v_min_u32", "v_max_u32"))),
                sum(n for name, n in o.items() if name.startswith("v_cndmask")), sum(n for name, n in o.items() if name.startswith("v_readlane")),
                k["salu"], k["lds"], k["vmem"], k["nop"]))
    print("total %d: " % sum(tot.values()) + ", ".join("%s %d" % kv for kv in sorted(tot.items())))
    print("most frequent: " + ", ".join("%s %d" % kv for kv in ops.most_common(24)))


if __name__ == "__main__":
    main()
