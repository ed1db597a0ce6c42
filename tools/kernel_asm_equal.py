#!/usr/bin/env python3
"""Are the device functions of two `hipcc --cuda-device-only -S` outputs the same?

    kernel_asm_equal.py before.s after.s

Each file is split at its function symbols; per symbol, the text from `.type SYM,@function` to `.size SYM` -- the instructions and,
for a kernel, its .amdhsa_kernel block -- is compared.  The order of the functions in the file follows the order of instantiation and
may differ; so may the function's index inside local labels (.LBB12_3, .Lfunc_end12) and inside the comments that name a block
(`in Loop: Header=BB12_2`, `Child Loop BB12_27`), which is masked (with the padding in front of a comment, which follows the label's length), and the lines that carry the per-compile
`__hip_cuid_<hash>` symbol.  Reads assembly for equality only.  Exit status 0 = same symbols, same bodies."""
import re
import sys

LOCAL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+(_\d+)?\b")
PAD = re.compile(r"[ \t]+;")
TYPE = re.compile(r"^\s*\.type\s+(\S+),@function")
SIZE = re.compile(r"^\s*\.size\s+(\S+),")


def functions(path):
    out, sym, body = {}, None, []
    with open(path) as f:
        for line in f:
            if sym is None:
                m = TYPE.match(line)
                if m:
                    sym, body = m.group(1), []
                continue
            if "__hip_cuid_" in line:
                continue
            m = SIZE.match(line)
            if m and m.group(1) == sym:
                out[sym] = "".join(body)
                sym = None
            else:
                body.append(PAD.sub(" ;", LOCAL.sub(lambda k: k.group(1) + (k.group(2) or ""), line)))
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    differ = sorted(s for s in a if s in b and a[s] != b[s])
    kernels = sum(1 for s in a if ".amdhsa_kernel " + s in a[s])
    print("%d functions (%d kernels) in %s, %d in %s: %d only in the first, %d only in the second, %d differ"
          % (len(a), kernels, sys.argv[1], len(b), sys.argv[2], len(only_a), len(only_b), len(differ)))
    for s in only_a + only_b + differ:
        print("  " + s)
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    sys.exit(main())
