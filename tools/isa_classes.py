#!/usr/bin/env python3
"""tools/isa_classes.py FILE.s [NAME-REGEX] -- instruction classes per function of a gfx950 assembly listing (hipcc -S): the
VALU instructions as multiply-add / low or high product / carry (add and subtract with carry in or out) / move / select /
other, next to LDS, memory, scalar, s_nop and s_waitcnt counts.  Static counts: every branch of a function is counted once."""
import collections
import re
import sys

VALU = ("mad", "mul", "carry", "move", "select", "valu_other")


def classify(op):
    if op.startswith("v_mad_u64"):
        return "mad"
    if op.startswith(("v_mul_lo", "v_mul_hi")):
        return "mul"
    if op.startswith(("v_addc", "v_subb", "v_add_co", "v_sub_co")):
        return "carry"
    if op.startswith(("v_mov", "v_accvgpr")):
        return "move"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith("v_"):
        return "valu_other"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "scratch_", "flat_")):
        return "vmem"
    if op.startswith("s_nop"):
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    return "salu"


def count(path, pattern):
    out, cur = collections.OrderedDict(), None
    for ln in open(path):
        g = re.match(r"^([A-Za-z_]\w*):", ln)
        if g and not g.group(1).startswith(("BB", "L")):
            cur = g.group(1) if re.search(pattern, g.group(1)) else None
            if cur:
                out[cur] = collections.Counter()
            continue
        if ln.startswith(".Lfunc_end"):
            cur = None
        t = ln.strip().split()
        if cur is None or not t or t[0].startswith((".", ";")) or t[0].endswith(":"):
            continue
        out[cur][classify(t[0])] += 1
    return out


def main():
    pattern = sys.argv[2] if len(sys.argv) > 2 else "."
    print("%-44s %5s | %5s %4s %5s %5s %6s %5s | %4s %4s %5s %7s" % (("function", "VALU") + VALU[:5] + ("other", "lds", "vmem", "s_nop", "waitcnt")))
    for name, c in count(sys.argv[1], pattern).items():
        print("%-44s %5d | %5d %4d %5d %5d %6d %5d | %4d %4d %5d %7d" % (
            name[:44], sum(c[k] for k in VALU), c["mad"], c["mul"], c["carry"], c["move"], c["select"], c["valu_other"], c["lds"], c["vmem"],
            c["s_nop"], c["waitcnt"]))


if __name__ == "__main__":
    main()
