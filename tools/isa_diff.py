#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of one kernel file, kernel by
kernel: the evidence that a source refactor left the generated code alone.

    python tools/isa_diff.py PARENT.s TREE.s
    python tools/isa_diff.py PARENT.hip TREE.hip [extra hipcc flags]

A .hip argument is compiled first with the Makefile's HIPFLAGS plus
`-Icsrc --cuda-device-only -S` (and any extra flags given).  Per kernel symbol
the tool compares
  * the instruction stream (comments, .file / .loc / .ident and the
    __hip_cuid_* lines dropped; the function index in local labels, which
    shifts when a kernel leaves the file, normalised: .LBB<n>_<m> -> .LBB_<m>),
  * the .amdhsa_* directives of its kernel descriptor,
  * its metadata entry (VGPR / SGPR / AGPR counts, spill counts, private
    segment, LDS, arguments).
It prints the kernels present on one side only and the kernels that differ,
and exits 1 if any kernel present on both sides differs."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_LABEL = re.compile(r"\.L(BB|JTI|func_begin|func_end|tmp)(\d+)(_\d+)?")
_DROP = re.compile(r"^\.(file|loc|ident|cfi_\w+)\b")


def makefile_hipflags():
    """HIPCC and HIPFLAGS as the Makefile sets them (ARCH expanded)."""
    var = {}
    for line in open(os.path.join(ROOT, "Makefile")):
        m = re.match(r"(\w+)\s*\?=\s*(.*)", line)
        if m:
            var[m.group(1)] = m.group(2).strip()
    flags = re.sub(r"\$\((\w+)\)", lambda m: var[m.group(1)], var["HIPFLAGS"])
    return os.environ.get("HIPCC", var["HIPCC"]), flags.split()


def assemble(src, extra):
    hipcc, flags = makefile_hipflags()
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.run([hipcc, *flags, "-I" + os.path.join(ROOT, "csrc"), *extra, "--cuda-device-only", "-S", "-o", out,
                    src], check=True)
    return out


def clean(line):
    """One assembly line without its comment, local-label indices normalised; '' if it carries nothing."""
    line = line.split(";", 1)[0].strip()
    if not line or _DROP.match(line) or "__hip_cuid_" in line:
        return ""
    return _LABEL.sub(lambda m: ".L%s%s" % (m.group(1), m.group(3) or ""), line)


def parse(path):
    """{kernel symbol: {"code": [...], "amdhsa": [...], "meta": [...]}}"""
    lines = open(path).read().split("\n")
    kernels = {}
    sym, part = None, None
    i = 0
    # kernel descriptors name the kernels; a function body runs from `SYM:` to its .Lfunc_end
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    for k in names:
        kernels[k] = {"code": [], "amdhsa": [], "meta": []}
    while i < len(lines):
        ln = lines[i]
        head = ln.split(";", 1)[0].rstrip()
        if part is None and head.endswith(":") and head[:-1] in names:
            sym, part = head[:-1], "code"
        elif part == "code" and re.match(r"\s*\.amdhsa_kernel\s", ln):
            part = "amdhsa"
        elif part == "amdhsa" and ".end_amdhsa_kernel" in ln:
            part = "tail"
        elif part == "tail" and "-- End function" in ln:
            part = "sets"
        elif part == "sets" and not re.match(r"\s*\.set\s", ln):
            sym, part = None, None
            continue
        elif part == "code":
            c = clean(ln)
            if c:
                kernels[sym]["code"].append(c)
        elif part == "amdhsa":
            kernels[sym]["amdhsa"].append(clean(ln))
        elif part == "sets":
            kernels[sym]["meta"].append(clean(ln))
        i += 1
    # metadata: one YAML entry per kernel under amdhsa.kernels
    try:
        b, e = lines.index("amdhsa.kernels:"), lines.index("\t.end_amdgpu_metadata")
    except ValueError:
        return kernels
    entry = []
    for ln in lines[b + 1:e] + ["  - "]:
        if ln.startswith("  - ") or not ln.startswith("    "):
            name = [x.split(":", 1)[1].strip() for x in entry if x.strip().startswith(".name:")]
            if name and name[0] in kernels:
                kernels[name[0]]["meta"] += [x.strip() for x in entry]
            entry = []
            if not ln.startswith("  - "):
                continue
        entry.append(ln[4:] if ln.startswith("  - ") else ln)
    return kernels


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b, extra = sys.argv[1], sys.argv[2], sys.argv[3:]
    made = []
    if a.endswith(".hip"):
        a = assemble(a, extra)
        made.append(a)
    if b.endswith(".hip"):
        b = assemble(b, extra)
        made.append(b)
    ka, kb = parse(a), parse(b)
    for f in made:
        os.remove(f)
    only_a, only_b = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    both = sorted(set(ka) & set(kb))
    differ = []
    for k in both:
        parts = [p for p in ("code", "amdhsa", "meta") if ka[k][p] != kb[k][p]]
        if parts:
            differ.append((k, parts))
    print("kernels: %d in parent, %d in tree, %d in both" % (len(ka), len(kb), len(both)))
    print("instructions compared: %d" % sum(len(ka[k]["code"]) for k in both))
    for title, ks in (("only in parent", only_a), ("only in tree", only_b)):
        print("%s: %d" % (title, len(ks)))
        for k in ks:
            print("  %s (%d lines)" % (k, len((ka if ks is only_a else kb)[k]["code"])))
    print("identical: %d" % (len(both) - len(differ)))
    print("different: %d" % len(differ))
    for k, parts in differ:
        print("  %s: %s (%d -> %d code lines)" % (k, ", ".join(parts), len(ka[k]["code"]), len(kb[k]["code"])))
        for p in parts:
            d = list(difflib.unified_diff(ka[k][p], kb[k][p], "parent", "tree", lineterm="", n=1))
            for ln in d[:40]:
                print("      " + ln)
            if len(d) > 40:
                print("      ... %d more diff lines" % (len(d) - 40))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
