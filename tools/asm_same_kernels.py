#!/usr/bin/env python3
"""Are two device-only assembly files (hipcc -S --cuda-device-only) the same kernels?  usage: asm_same_kernels.py A.s B.s

A host-side refactor may change the ORDER in which template kernels are instantiated, and with it the order of the functions in
the file and the function index inside local labels (.LBB<index>_<block>, .Lfunc_end<index>).  So: file-path / ident lines
dropped, the function index in local labels and the translation unit's __hip_cuid hash blanked, the file cut into chunks at
every section start and every entry of the metadata's kernel list, and the chunks compared as sorted lists.  Prints the counts; exit status 1 when they differ.

A kernel may also MOVE between two source files; then each side is the concatenation of both files' assembly.  For that the
cuts fall at every `.text` as well (a kernel that is no template is in .text, behind its predecessor's kernel info) and at the
end of the metadata's kernel list (its last entry is followed by the file's trailer), and what the assembler writes once per
file and section in use rather than per kernel is dropped: the line that places __hip_cuid in whichever section came last, a
bare section switch, and the padding that closes .text."""
import re
import sys


def chunks(path):
    out, cur = [], []
    for line in open(path):
        if re.match(r"\s*\.(file|ident)\b", line):
            continue
        line = re.sub(r"BB\d+_", "BB_", line)                                  # .LBB10_352, and "Header=BB10_352" in comments
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        line = re.sub(r":\s+;", ": ;", line)                                    # the comment column follows the label's width
        line = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", line)             # a hash of the translation unit's text
        if re.match(r"\t\.type\t__hip_cuid,", line):
            continue
        if re.match(r"\t\.section\b|\t\.text$|  - \.|amdhsa\.target:", line) and cur:
            out.append("".join(cur))
            cur = []
        cur.append(line)
    out.append("".join(cur))
    return [c for c in out if not re.fullmatch(r"\t\.(text|section\t\S+)\n(\t\.p2alignl .*\n\t\.fill .*\n)?", c)]


a, b = chunks(sys.argv[1]), chunks(sys.argv[2])
same_order = a == b
sa, sb = sorted(a), sorted(b)
kernels = lambda cs: sorted(set(m for c in cs for m in re.findall(r"^\t\.amdhsa_kernel (\S+)", c, flags=re.M)))
print("%s: %d chunks, %d kernels; %s: %d chunks, %d kernels; identical in file order: %s; identical as sorted chunks: %s; "
      "same kernel symbols: %s" % (sys.argv[1], len(a), len(kernels(a)), sys.argv[2], len(b), len(kernels(b)), same_order, sa == sb,
                                   kernels(a) == kernels(b)))
if sa != sb:
    only_a = [c for c in sa if c not in set(sb)]
    only_b = [c for c in sb if c not in set(sa)]
    print("chunks only in A: %d, only in B: %d" % (len(only_a), len(only_b)))
    for c in (only_a[:2] + only_b[:2]):
        print("----\n" + c[:600])
    sys.exit(1)
