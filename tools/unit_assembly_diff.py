#!/usr/bin/env python3
"""tools/unit_assembly_diff.py [--common] A.s B.s — are two device assemblies of a unit (hipcc
--cuda-device-only -S) the same functions, whatever order they come in?

Prints `identical` when the files are equal byte for byte.  Otherwise the files are cut at
every function's begin marker, and their tails (data objects, the metadata's kernel
entries) at every object; each function of A must be B's function of the same name line
for line, and the tails must hold the same objects.  The only text that depends on a
function's position is the function number inside its local labels (.LBB<n>_<k>,
.LJTI<n>_<k>, .Lfunc_end<n>, and BB<n>_<k> in the loop comments), which is dropped before comparing, with the padding between a label and its comment.  --common compares the functions both
files hold and names the others (a unit that left some kernels to another unit).  Exit status
1 on any difference inside a function or an object."""
import collections
import re
import sys

BEGIN = re.compile(r"^\t\.globl\t(\S+)\s*; -- Begin function")
TAIL = re.compile(r"^\t\.section\t\.AMDGPU\.gpr_maximums")
OBJECT = re.compile(r"^\t\.type\t\S+,@object|^  - \.agpr_count|^amdhsa\.target|^\t\.amdgpu_metadata")
PAD = re.compile(r"(?<=:) +;")   # a label's comment column moves with the label's length
LABEL = re.compile(r"(\.LJTI|\.Lfunc_begin|\.Lfunc_end|(?<![A-Za-z0-9_])BB|\.LBB)\d+")


def cut(path):
    lines = [PAD.sub(" ;", LABEL.sub(r"\1", l)) for l in open(path).read().split("\n")]
    tail = next(i for i, l in enumerate(lines) if TAIL.match(l))
    starts = [(i - 1, m.group(1)) for i, l in enumerate(lines[:tail]) if (m := BEGIN.match(l))]
    funcs = {}
    for (at, name), (end, _) in zip(starts, starts[1:] + [(tail, None)]):
        assert name not in funcs, name
        funcs[name] = lines[at:end]
    marks = [i for i in range(tail, len(lines)) if OBJECT.match(lines[i])]
    objects = ["\n".join(lines[a:b]) for a, b in zip([tail] + marks, marks + [len(lines)])]
    return lines[:starts[0][0]], [n for _, n in starts], funcs, collections.Counter(objects)


def main():
    common = "--common" in sys.argv
    a, b = [x for x in sys.argv[1:] if x != "--common"]
    if open(a, "rb").read() == open(b, "rb").read():
        print("identical")
        return 0
    head_a, order_a, fa, oa = cut(a)
    head_b, order_b, fb, ob = cut(b)
    only = sorted(set(fa) ^ set(fb))
    bad = [n for n in fa if n in fb and fa[n] != fb[n]]
    if common:
        print(f"in one file only: {only}")
        fa = {n: f for n, f in fa.items() if n in fb}
        oa = ob = collections.Counter()
    else:
        bad += only
        if head_a != head_b:
            bad.append("<file head>")
        if oa != ob:
            bad.append("<data objects / kernel metadata>")
    moved = sum(1 for x, y in zip(order_a, order_b) if x != y)
    print(f"{len(fa)} functions, {sum(map(len, fa.values()))} lines in them; {moved} at another position; "
          f"{sum(oa.values())} data objects and metadata entries; " +
          (f"DIFFERENT: {bad}" if bad else "every function and object line for line the same (function numbers of local labels aside)"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
