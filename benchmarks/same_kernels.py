"""Are the kernels of two builds the same code?  python benchmarks/same_kernels.py A.s B.s

A.s and B.s are the device assembly of one source at two commits (hipcc's flags of _lib.py plus `--cuda-device-only -S`).
Each is split into functions at `; -- Begin function NAME` ... `; -- End function`, which holds the instructions and the
.amdhsa_* descriptor. Comments are dropped and every local label (.L...) becomes one token:
labels are numbered by the function's position in the file, which a reordering of the host code changes. Prints the symbols
only in A, only in B and those whose text differs; exits 0 only if there are none and both files hold functions (a host-only or
otherwise wrong file is not "the same kernels"). Reads the two files and nothing else.

What it does not see: since every local label is one token, a branch retargeted to another block of the same function; and
whatever lies outside Begin ... End (the per-symbol .set lines, the metadata note). Registers, scratch and LDS are in the
descriptor and are compared; libnaf_hip.so.usage.json is the second check of them.
"""
import re
import sys


def functions(path):
    out, name = {}, None
    with open(path) as f:
        for line in f:
            m = re.search(r"; -- Begin function (\S+)", line)
            if m:
                name = m.group(1)
                out[name] = []
            if name is not None and "; -- End function" in line:
                name = None
            line = re.sub(r"\.L\w+", ".L", line.split(";", 1)[0]).strip()
            if name is not None and line:
                out[name].append(line)
    return out


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    a, b = functions(argv[1]), functions(argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    print(f"{len(a)} functions in A ({sum(map(len, a.values()))} lines), {len(b)} in B ({sum(map(len, b.values()))} lines)")
    for title, names in (("only in A", only_a), ("only in B", only_b), ("differing", differ)):
        print(f"{title}: {len(names)}")
        for k in names:
            print("   ", k)
    for k in differ[:3]:      # where the first few part ways
        i = next((i for i, (x, y) in enumerate(zip(a[k], b[k])) if x != y), min(len(a[k]), len(b[k])))
        print(f"{k} line {i}:\n  A: {a[k][i:i + 1]}\n  B: {b[k][i:i + 1]}")
    if not a or not b:
        print("no function found in " + " and ".join(n for n, f in (("A", a), ("B", b)) if not f) + ": not device assembly of a build?")
    return 1 if only_a or only_b or differ or not a or not b else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
