#!/usr/bin/env python3
"""Instruction mix of one gfx950 kernel, region by region: where the issue
slots of a loop go.  Runs on the CPU (it reads compiler output only).

    python tools/isa_loop_stats.py FILE.s   'x3_dense_fused3_kernel<7>'
    python tools/isa_loop_stats.py FILE.hip 'x3_dense_fused3_kernel<7>' [extra hipcc flags]
    python tools/isa_loop_stats.py FILE.s   --list

A .hip argument is compiled first exactly as tools/isa_diff.py compiles it.
The kernel is named by its mangled symbol, by its demangled name or by a
substring that matches one kernel only (template arguments as c++filt prints
them: `name<7>`).

A region is a maximal run of basic blocks with the same loop nesting: the code
between two labels that some branch of the kernel targets (or from a loop's
back edge to the next such label).  A loop is the label
range [target, branch] of a backward branch; `depth` counts the loops a region
lies in and `loop` names the innermost one by its head label.  Per region:

  mfma   v_mfma_* / v_smfmac_*
  valu   every other v_* instruction (of which `mul`: v_mul_lo / v_mul_hi /
         v_mad_u64_u32, the quarter-rate integer multiplies; `cnd`: v_cndmask;
         `cvt`: v_cvt_*)
  lds    ds_*
  vmem   global_* / buffer_* / flat_* / scratch_*
  salu   s_* except s_waitcnt, s_barrier and s_nop
  wait   s_waitcnt*
  bar    s_barrier

and, for the kernel, the VGPR / AGPR / SGPR counts, the spill counts and the
scratch size from its metadata.  --min N hides regions of fewer than N
instructions (default 8); --json prints one JSON object instead of the table."""
import argparse
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_diff  # noqa: E402

_BRANCH = re.compile(r"^s_c?branch\w*\s+(\S+)")
_LABEL = re.compile(r"^(\.L\w+):$")
COLS = ("mfma", "valu", "mul", "cnd", "cvt", "lds", "vmem", "salu", "wait", "bar")


def classify(op):
    """The columns one opcode counts in."""
    if op.startswith(("v_mfma", "v_smfmac")):
        return ("mfma",)
    if op.startswith("v_"):
        extra = ()
        if op.startswith(("v_mul_lo", "v_mul_hi", "v_mad_u64_u32", "v_mad_i64_i32")):
            extra = ("mul",)
        elif op.startswith("v_cndmask"):
            extra = ("cnd",)
        elif op.startswith("v_cvt"):
            extra = ("cvt",)
        return ("valu",) + extra
    if op.startswith("ds_"):
        return ("lds",)
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return ("vmem",)
    if op.startswith("s_waitcnt"):
        return ("wait",)
    if op == "s_barrier":
        return ("bar",)
    if op.startswith("s_") and op != "s_nop":
        return ("salu",)
    return ()


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short_name(pretty):
    """`void (anonymous namespace)::k<7>((anonymous namespace)::P)` -> `k<7>`"""
    return re.sub(r"^void |\(.*$", "", pretty.replace("(anonymous namespace)::", ""))


def pick(kernels, want):
    pretty = demangle(sorted(kernels))
    if want in kernels:
        return want, pretty
    short = {k: short_name(v) for k, v in pretty.items()}
    hits = [k for k, v in short.items() if v == want] or [k for k, v in pretty.items() if want in v]
    if len(hits) != 1:
        sys.exit("%r names %d kernels%s" % (want, len(hits), ": " + ", ".join(short[h] for h in hits[:8]) if hits else ""))
    return hits[0], pretty


def regions(code):
    """[(first label or '<entry>', depth, loop head or '', {col: n}, total)] in program order."""
    labels = {m.group(1): i for i, ln in enumerate(code) for m in [_LABEL.match(ln)] if m}
    targets, loops = set(), []
    for i, ln in enumerate(code):
        m = _BRANCH.match(ln)
        if m and m.group(1) in labels:
            targets.add(m.group(1))
            if labels[m.group(1)] <= i:
                loops.append((labels[m.group(1)], i, m.group(1)))
    out, cur = [], None

    def nest(i):
        inside = sorted((l for l in loops if l[0] <= i <= l[1]), key=lambda l: l[1] - l[0])
        return len(inside), inside[0][2] if inside else ""
    for i, ln in enumerate(code):
        m = _LABEL.match(ln)
        if m:
            if m.group(1) in targets or cur is None:
                cur = [m.group(1), *nest(i), dict.fromkeys(COLS, 0), 0]
                out.append(cur)
            continue
        if cur is None:
            cur = ["<entry>", *nest(i), dict.fromkeys(COLS, 0), 0]
            out.append(cur)
        elif (cur[1], cur[2]) != nest(i):  # fell out of a loop behind its back edge
            cur = ["<past %s>" % cur[2].replace(".LBB", ""), *nest(i), dict.fromkeys(COLS, 0), 0]
            out.append(cur)
        if ln.startswith("."):
            continue
        cols = classify(ln.split()[0])
        for c in cols:
            cur[3][c] += 1
        cur[4] += 1
    return [tuple(r) for r in out]


def meta(lines):
    want = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count",
            "private_segment_fixed_size", "group_segment_fixed_size")
    got = {}
    for ln in lines:
        m = re.match(r"\.(\w+):\s*(\d+)$", ln)
        if m and m.group(1) in want:
            got[m.group(1)] = int(m.group(2))
    return got


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("file")
    ap.add_argument("kernel", nargs="?")
    ap.add_argument("--list", action="store_true", help="list the kernels with their register and spill figures")
    ap.add_argument("--min", type=int, default=8)
    ap.add_argument("--json", action="store_true")
    a, extra = ap.parse_known_args()
    path, made = a.file, False
    if path.endswith(".hip"):
        path, made = isa_diff.assemble(path, extra), True
    kernels = isa_diff.parse(path)
    if made:
        os.remove(path)
    if a.list or not a.kernel:
        pretty = demangle(sorted(kernels))
        for k in sorted(kernels, key=lambda k: pretty[k]):
            m = meta(kernels[k]["meta"])
            print("%-70s vgpr %3d agpr %3d sgpr %3d spill %d scratch %d B" % (
                short_name(pretty[k]), m.get("vgpr_count", -1), m.get("agpr_count", 0),
                m.get("sgpr_count", -1), m.get("vgpr_spill_count", -1), m.get("private_segment_fixed_size", -1)))
        return 0
    sym, pretty = pick(kernels, a.kernel)
    regs = regions(kernels[sym]["code"])
    total = dict.fromkeys(COLS, 0)
    for r in regs:
        for c in COLS:
            total[c] += r[3][c]
    m = meta(kernels[sym]["meta"])
    if a.json:
        print(json.dumps({"kernel": pretty[sym], "meta": m, "total": total, "regions": [
            {"label": r[0], "depth": r[1], "loop": r[2], "instructions": r[4], **r[3]} for r in regs]}))
        return 0
    print(pretty[sym])
    print("  " + "  ".join("%s %d" % (k.replace("_count", "").replace("_fixed_size", ""), v) for k, v in m.items()))
    print("%-12s %5s %-10s %6s " % ("region", "depth", "loop", "instr") + " ".join("%5s" % c for c in COLS))
    for r in regs:
        if r[4] >= a.min:
            print("%-12s %5d %-10s %6d " % (r[0], r[1], r[2], r[4]) + " ".join("%5d" % r[3][c] for c in COLS))
    print("%-12s %5s %-10s %6d " % ("total", "", "", sum(r[4] for r in regs)) + " ".join("%5d" % total[c] for c in COLS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
