#!/usr/bin/env python3
"""Count the instructions one wave issues along a given path through a kernel's gfx950 assembly.

    hipcc -S ... ragen_amd/csrc/sokoban.hip -o sokoban.s        (the project's flags, device side)
    tools/asm_path_count.py sokoban.s KERNEL DECISIONS

KERNEL is a substring of the kernel's mangled name (the first kernel label containing it is
taken).  DECISIONS is a text file that tells the walk what the wave does at every conditional
branch it meets, in the order it meets them:

    T            the branch is taken
    N            it falls through
    @LABEL name  when the walk reaches LABEL (e.g. @.LBB14_12 steps) a new segment starts
    # ...        comment

The walk starts at the kernel's label in a segment called "entry", follows s_branch, applies the
next decision at each s_cbranch_*, and stops at s_endpgm.  A loop is walked as often as the
decisions say.  Printed: per segment and for the whole path the number of instructions and their
classes (VALU, SALU, VMEM, SMEM, LDS, wait/nop, branch).  Used for DESIGN.md §3.1 item 13; the
decision files of the bench kernels are in tools/asm_paths/."""
import re
import sys

CLASSES = ("VALU", "SALU", "VMEM", "SMEM", "LDS", "wait", "branch")


def classify(op):
    if op in ("s_waitcnt", "s_nop") or op.startswith("s_waitcnt") or op == "s_sleep":
        return "wait"
    if op.startswith(("s_branch", "s_cbranch", "s_endpgm", "s_setpc", "s_swappc")):
        return "branch"
    if op.startswith(("s_load", "s_memtime", "s_memrealtime")):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "VMEM"
    if op.startswith("v_"):
        return "VALU"
    raise SystemExit(f"unclassified instruction {op!r}")


def parse(path, kernel):
    """-> (list of (op, operands), {label: index}) of the first kernel whose name contains `kernel`."""
    lines = open(path).read().split("\n")
    start = None
    for i, ln in enumerate(lines):
        if ln.endswith(":") or re.match(r"^[\w.$]+:\s*;", ln):
            name = ln.split(":")[0]
            if kernel in name and not name.startswith("."):
                start = i
                break
    if start is None:
        raise SystemExit(f"no kernel label containing {kernel!r}")
    ins, labels = [], {}
    for ln in lines[start + 1:]:
        code = ln.split(";")[0].rstrip()
        if not code.strip():
            continue
        m = re.match(r"^([\w.$]+):", code)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        tok = code.split(None, 1)
        op = tok[0]
        if op == ".end_amdhsa_kernel" or op.startswith(".Lfunc_end"):
            break
        if op.startswith("."):
            continue
        ins.append((op, tok[1] if len(tok) > 1 else ""))
    return ins, labels


def walk(ins, labels, decisions, marks):
    segs, order = {}, []

    def seg(name):
        if name not in segs:
            segs[name] = dict.fromkeys(CLASSES, 0)
            order.append(name)
        return segs[name]

    at = {labels[k]: v for k, v in marks.items() if k in labels}
    missing = [k for k in marks if k not in labels]
    if missing:
        raise SystemExit(f"segment labels not in the kernel: {missing}")
    cur = seg("entry")
    pc, d = 0, 0
    while True:
        if pc in at:
            cur = seg(at[pc])
        if pc >= len(ins):
            raise SystemExit("fell off the kernel's end")
        op, args = ins[pc]
        cur[classify(op)] += 1
        if op == "s_endpgm":
            break
        if op == "s_branch":
            pc = labels[args.strip()]
        elif op.startswith("s_cbranch"):
            if d >= len(decisions):
                ctx = "\n".join(f"    {o} {a}" for o, a in ins[max(0, pc - 8):pc + 1])
                here = [k for k, v in labels.items() if v <= pc]
                raise SystemExit(f"decision {d + 1} missing (after label {max(here, key=labels.get) if here else '-'}):\n{ctx}")
            pc = labels[args.strip()] if decisions[d] == "T" else pc + 1
            d += 1
        else:
            pc += 1
    if d != len(decisions):
        raise SystemExit(f"{len(decisions) - d} decisions left over")
    return segs, order


def main(argv):
    if len(argv) != 4:
        raise SystemExit(__doc__)
    ins, labels = parse(argv[1], argv[2])
    decisions, marks = [], {}
    for ln in open(argv[3]):
        ln = ln.split("#")[0].strip()
        if not ln:
            continue
        if ln.startswith("@"):
            lab, name = ln[1:].split(None, 1)
            marks[lab] = name
        elif ln in ("T", "N"):
            decisions.append(ln)
        else:
            raise SystemExit(f"bad decision line {ln!r}")
    segs, order = walk(ins, labels, decisions, marks)
    total = dict.fromkeys(CLASSES, 0)
    print(f"{'segment':<28}{'instr':>6}" + "".join(f"{c:>7}" for c in CLASSES))
    for name in order + ["whole path"]:
        row = total if name == "whole path" else segs[name]
        if name != "whole path":
            for c in CLASSES:
                total[c] += row[c]
        print(f"{name:<28}{sum(row.values()):>6}" + "".join(f"{row[c]:>7}" for c in CLASSES))


if __name__ == "__main__":
    main(sys.argv)
