#!/usr/bin/env python3
"""Are the kernels of two builds the same instructions?

    hipcc <build.py's flags of the file> --cuda-device-only -S -o A.s csrc/<file>.hip      (once per file and build)
    python tools/isa_same.py A1.s[,A2.s...] B1.s[,B2.s...]

Splits the listings of each side by function symbol (several files per side: code may move between translation units), drops
what only numbers a function inside its file (the index in .LBB<k>_ / BB<k>_ / .Ltmp<k> / .Lfunc_*<k>) and the compilation
unit's id symbol, and prints every function whose text differs or that one side lacks.  Exit status 1 if there is one.
"""
import re
import sys

LOCAL = re.compile(r'(\.?L?BB)\d+(?=_)|(\.Ltmp)\d+|(\.Lfunc_[a-z]+)\d+')


def functions(paths):
    out = {}
    for path in paths.split(','):
        name = None
        for line in open(path):
            m = re.match(r'\s+\.type\s+(\S+),@function', line)
            if m:
                name = m.group(1)
                out[name] = []
            elif name is not None and '__hip_cuid_' not in line:
                # blanks collapsed: the column of a trailing comment moves with the width of the index
                out[name].append(LOCAL.sub(lambda g: next(x for x in g.groups() if x), ' '.join(line.split())))
                if line.startswith('.Lfunc_end'):
                    name = None
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = ['only in %s: %s' % (sys.argv[1 + (n in b)], n) for n in sorted(set(a) ^ set(b))]
    bad += ['differs: %s' % n for n in sorted(set(a) & set(b)) if a[n] != b[n]]
    print('\n'.join(bad + ['%d functions on one side, %d on the other, %d differ or are missing' % (len(a), len(b), len(bad))]))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
