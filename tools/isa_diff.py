"""Kernel-by-kernel equality of two hipcc -S (--cuda-device-only) gfx950 assembly files.

  python tools/isa_diff.py <a.s> <b.s> [--list] [--rename-a OLD NEW]

Splits both files by kernel symbol (every .amdhsa_kernel name). A kernel's text is its
instructions (from its label to .Lfunc_end) plus its .amdhsa_kernel descriptor (registers,
scratch, LDS, kernarg size). Normalised is only what necessarily moves when code is
rearranged in the source: the function index inside local labels (.LBB<n>_, .Lfunc_end<n>, and
the same BB<n>_ label named in a block comment), and the padding between a label and its comment, whose
column depends on how many digits <n> has.
Lines outside kernels (.file, .ident, the __hip_cuid_* symbol, metadata) are not compared. A device
function that is not inlined would be a symbol of its own outside every kernel: such symbols
(.type <sym>,@function without a descriptor) are counted and, if there are any, fail the run.
Prints the number of kernels compared, the symbols present on one side only and the symbols
that differ; exit status 1 unless all three are empty. It looks at nothing but equality.
--rename-a OLD NEW: for a change that renames kernels (a template parameter dropped: the argument
list is part of the mangled name), re.sub(OLD, NEW) is applied to the text of <a.s> before
anything else, so to the symbol names and to wherever they stand in the compared text; OLD should
be written to match inside those symbol names only. The rule is printed with the result.
"""
import re
import sys


def kernels(path, rename=None):
    text = open(path).read()
    if rename:
        text = re.sub(rename[0], rename[1], text)
    lines = text.split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    want = set(names)
    funcs = [m.group(1) for m in (re.match(r"\s*\.type\s+([^,\s]+),@function", l) for l in lines) if m]
    others = sorted(set(funcs) - want)
    out = {n: [] for n in names}
    cur, mode = None, None
    for l in lines:
        s = l.strip()
        if cur is None:
            head = l.split(":", 1)[0]  # "<symbol>:   ; @<symbol>"
            if ":" in l and head in want:
                cur, mode = head, "text"
            elif s.startswith(".amdhsa_kernel "):
                cur, mode = s.split()[1], "desc"
                out[cur].append(s)
            continue
        if mode == "text" and l.startswith(".Lfunc_end"):
            cur = None
            continue
        # .LBB<n>_<k> (and BB<n>_<k> in the block comments), .Lfunc_end<n>: <n> is the function's index
        # (and the padding in front of a label's comment, whose column moves with the digits of <n>)
        out[cur].append(re.sub(r"^(\.LBB_\d+:)\s*;", r"\1 ;", re.sub(r"(\.LBB|\bBB|\.Lfunc_end)\d+", r"\1", l)))
        if mode == "desc" and s == ".end_amdhsa_kernel":
            cur = None
    return out, others


def main():
    rename = None
    if "--rename-a" in sys.argv:
        i = sys.argv.index("--rename-a")
        rename = (sys.argv[i + 1], sys.argv[i + 2])
        print(f"rename rule for {sys.argv[1]}: {rename[0]} -> {rename[1]}")
    (a, oa), (b, ob) = kernels(sys.argv[1], rename), kernels(sys.argv[2])
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    differ = [n for n in both if a[n] != b[n]]
    print(f"kernels compared: {len(both)}")
    print(f"only in {sys.argv[1]}: {len(only_a)}")
    for n in only_a:
        print("   ", n)
    print(f"only in {sys.argv[2]}: {len(only_b)}")
    for n in only_b:
        print("   ", n)
    print(f"function symbols that are not kernels (not compared): {len(oa)} / {len(ob)}")
    for n in sorted(set(oa) | set(ob)):
        print("   ", n)
    print(f"differing: {len(differ)}")
    for n in differ:
        k = next((i for i, (x, y) in enumerate(zip(a[n], b[n])) if x != y), min(len(a[n]), len(b[n])))
        print(f"    {n}  (first difference at line {k} of {len(a[n])} / {len(b[n])})")
    if "--list" in sys.argv:
        for n in both:
            print("  =" if a[n] == b[n] else "  !", n)
    sys.exit(1 if only_a or only_b or differ or oa or ob else 0)


if __name__ == "__main__":
    main()
