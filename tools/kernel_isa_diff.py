"""Are the kernels of two device-side assembly listings the same?  For refactors of host code:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -Iinclude -o A.s fqcomp28_amd/csrc/encode.hip   (at each commit)
    python3 tools/kernel_isa_diff.py A.s B.s
Whole-file equality is too strict: reordering host calls changes the order in which templates are instantiated, and with it
the order of the functions in the file and the function index inside .LBB<i>_<j> labels.  So, per kernel, by mangled name:
the body from `.type NAME,@function` to `.Lfunc_endN:` with comments stripped, .LBB<i>_<j> rewritten to .LBB_<j> and blank
lines dropped, and the `.amdhsa_kernel NAME ... .end_amdhsa_kernel` descriptor block.  Prints the kernels that differ or
exist on one side only and exits non-zero if there are any.  It compares; it looks for no instruction."""
import re
import sys


def kernels(path):
    """-> {kernel name: (normalised body, descriptor block)}"""
    text = open(path).read()
    bodies = {}
    for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        lines = (re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", re.sub(r";.*", "", ln)).rstrip() for ln in m.group(2).splitlines())
        bodies[m.group(1)] = "\n".join(ln for ln in lines if ln.strip())
    descs = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)}
    return {name: (bodies.get(name), d) for name, d in descs.items()}


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print("only in %s: %s" % (sys.argv[2] if name not in a else sys.argv[1], name))
        elif a[name][0] is None or b[name][0] is None:
            print("no body found: %s" % name)
        elif a[name][0] != b[name][0]:
            print("body differs: %s" % name)
        elif a[name][1] != b[name][1]:
            print("descriptor differs: %s" % name)
        else:
            continue
        bad += 1
    print("%d kernels in %s, %d in %s, %d differ" % (len(a), sys.argv[1], len(b), sys.argv[2], bad))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
