#!/usr/bin/env python3
"""Build a scratch libtcamd_hip variant into the git-ignored k12ab/ for an A/B
against the production build (tools/probes/lib_ab.sh): one translation unit
compiled in place of a production object and linked with the tree's other
kernel objects (make must have run).  Two forms:

    python tools/probes/build_variant.py NAME csrc/kernels/densenet_x3.hip 'OLD=>NEW' ['OLD2=>NEW2' ...]

a production kernel source with literal text replacements applied in a
temporary copy (each OLD must occur exactly once; \\n in OLD / NEW is a
newline), linked instead of its own object; and

    python tools/probes/build_variant.py --unit NAME tools/probes/k11w.hip [--replaces densenet_x3] ['OLD=>NEW' ...]

a whole replacement translation unit: a probe file that #includes the
production source and adds to it, linked instead of build/*/<replaces>.o
(default densenet_x3).  Both write k12ab/libtcamd_hip_NAME.so."""
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
HIPCC = "/opt/rocm/bin/hipcc"


def patch(text, reps):
    for rep in reps:
        old, new = (t.replace("\\n", "\n") for t in rep.split("=>", 1))
        assert text.count(old) == 1, "%r occurs %d times" % (old, text.count(old))
        text = text.replace(old, new)
    return text


def build(name, src, text, replaces):
    """Compile `text` (a variant of the file `src`) and link it in place of build/*/<replaces>.o."""
    tmp = os.path.join(os.path.dirname(src), "_variant_%s.hip" % name)
    obj = "/tmp/_variant_%s.o" % name
    try:
        open(tmp, "w").write(text)
        subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "csrc"),
                        "-c", "-o", obj, tmp], check=True)
    finally:
        os.remove(tmp)
    objs = glob.glob(os.path.join(ROOT, "build/*/*.o"))
    assert any(os.path.basename(o) == replaces + ".o" for o in objs), "build/*/%s.o is missing: run make" % replaces
    objs = [o for o in objs if os.path.basename(o) != replaces + ".o"]
    os.makedirs(os.path.join(ROOT, "k12ab"), exist_ok=True)
    lib = os.path.join(ROOT, "k12ab", "libtcamd_hip_%s.so" % name)
    subprocess.run([HIPCC, "-shared", "-fPIC", "--offload-arch=gfx950", "-o", lib, obj, *objs, "-L/opt/rocm/lib",
                    "-lamdhip64"], check=True)
    return lib


def main():
    args = sys.argv[1:]
    unit = args[:1] == ["--unit"]
    if unit:
        args = args[1:]
    name, src = args[0], os.path.join(ROOT, args[1])
    args = args[2:]
    replaces = os.path.splitext(os.path.basename(src))[0]
    if unit:
        replaces = "densenet_x3"
        if args[:1] == ["--replaces"]:
            replaces, args = args[1], args[2:]
    print(build(name, src, patch(open(src).read(), args), replaces))


if __name__ == "__main__":
    main()
