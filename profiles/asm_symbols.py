#!/usr/bin/env python3
"""Compare two files of device assembly (hipcc --cuda-device-only -S) function by function.

    python profiles/asm_symbols.py before.s after.s

A function is the text from its label to its .Lfunc_end label, kernel descriptor included.  Block labels (.LBB12_3, .Lfunc_end12,
.LJTI12_0, ...) carry the function's number in the file and the __hip_cuid_ marker a hash of the build: both are renamed, comments
are dropped, and what is left is compared as a whole.  Reports the symbols only one file has, the number of identical ones, and for
each that differs: instruction lines, next_free_vgpr, next_free_sgpr, private_segment_fixed_size and static LDS bytes of both.
Exit status 0 when both files hold the same symbols and all are identical, else 1.
"""
import re
import sys

LABEL = re.compile(r"\.L([A-Za-z_]+?)\d+(_\d+)?\b")
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")
FIELDS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size")


def functions(path):
    """{symbol: normalised lines} of every @function symbol of the file"""
    out, name, body = {}, None, []
    pending = set()
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].rstrip()
        if not line:
            continue
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            pending.add(m.group(1))
            continue
        if name is None:
            if line.endswith(":") and line[:-1] in pending:
                name, body = line[:-1], []
            continue
        if line.startswith(".Lfunc_end"):
            out[name] = body
            name = None
            continue
        body.append(CUID.sub("__hip_cuid_", LABEL.sub(lambda m: ".L%sN%s" % (m.group(1), m.group(2) or ""), line)))
    return out


def figures(body):
    """(instruction lines, vgpr, sgpr, scratch bytes, static LDS bytes); descriptor fields are None for a plain device function"""
    code = body[:next((i for i, l in enumerate(body) if l.lstrip().startswith(".section")), len(body))]
    ins = sum(1 for l in code if l[:1] in "\t " and not l.lstrip().startswith(".") and not l.rstrip().endswith(":"))
    vals = {}
    for l in body:
        m = re.match(r"\s*\.amdhsa_(\w+)\s+(\S+)", l)
        if m and m.group(1) in FIELDS:
            vals[m.group(1)] = m.group(2)
    return (ins,) + tuple(vals.get(f) for f in FIELDS)


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    common = sorted(set(a) & set(b))
    differ = [s for s in common if a[s] != b[s]]
    print("symbols: %d in %s, %d in %s, %d in both" % (len(a), sys.argv[1], len(b), sys.argv[2], len(common)))
    for s in only_a:
        print("only in %s: %s" % (sys.argv[1], s))
    for s in only_b:
        print("only in %s: %s" % (sys.argv[2], s))
    print("identical up to labels: %d of %d" % (len(common) - len(differ), len(common)))
    if differ:
        print("differ (first file -> second file): instructions, vgpr, sgpr, scratch, lds")
        for s in differ:
            fa, fb = figures(a[s]), figures(b[s])
            print("  %s: %s" % (s, ", ".join("%s -> %s" % (x, y) for x, y in zip(fa, fb))))
    return 1 if (only_a or only_b or differ) else 0


if __name__ == "__main__":
    sys.exit(main())
