#!/usr/bin/env python3
"""Compare two device assemblies of the library (the output of tools/isa.sh's hipcc line for two trees) kernel by kernel.

A host-only change still moves the text: clang emits a kernel TEMPLATE's instantiation where the host code first names it, so
moving a launch reorders the kernels, renumbers their block labels (BB<function>_<block>, .Lfunc_end<function>) and the
columns of the comments behind them.  This prints whether every kernel's text is the same once those numbers are masked, and
whether the lines outside the kernels are the same multiset.

usage: isa_compare.py PARENT.s BRANCH.s
"""
import json
import re
import sys


def load(path):
    kernels, rest, cur, name = {}, [], None, None
    for line in open(path):
        if line.startswith(("\t.file", "\t.ident")):
            continue
        line = re.sub(r"\.L(func_end|func_begin|tmp)\d+", r".L\1N", line)
        line = re.sub(r"BB\d+_", "BBN_", line)
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", line)
        line = re.sub(r":\s+;", ": ;", line)
        if cur is None and re.match(r"\t\.(protected|section\t\.text\.)", line):
            cur = [line]
        elif cur is not None:
            cur.append(line)
            m = re.match(r"(\S+): ; @", line)
            if m:
                name = m.group(1)
            if line.startswith("; COMPUTE_PGM_RSRC2:TIDIG_COMP_CNT"):   # the last line of a kernel's resource comments
                kernels[name] = "".join(cur)
                cur = name = None
        else:
            rest.append(line)
    return kernels, rest


a, rest_a = load(sys.argv[1])
b, rest_b = load(sys.argv[2])
differing = sorted(set(a) ^ set(b)) + [k for k in a if k in b and a[k] != b[k]]
print(json.dumps({"kernels_parent": len(a), "kernels_branch": len(b), "kernels_differing": differing,
                  "lines_outside_kernels": len(rest_a), "lines_outside_kernels_same_multiset": sorted(rest_a) == sorted(rest_b)}))
sys.exit(1 if differing or sorted(rest_a) != sorted(rest_b) else 0)
