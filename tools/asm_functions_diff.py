#!/usr/bin/env python3
"""Compare the device functions of two builds of one HIP source, function by function: the gfx950 assembly hipcc keeps with -save-temps=obj
(<name>-hip-amdgcn-amd-amdhsa-gfx950.s).  Comments are dropped; what a function's POSITION in the file decides is normalised (the numbers of the local labels .LBB<n>_ and
.Lpost_getpc<n>); --drop REGEX (repeatable) removes a piece of every mangled name first, e.g. a template argument the newer build appended with its default value.
Prints one line per function of the OLDER build (lines, differing lines) and the functions only the newer build has.
usage: asm_functions_diff.py old.s new.s [--drop REGEX ...] [output.txt]"""
import difflib
import re
import sys


def functions(path, drops):
    text = open(path).read()
    for d in drops:
        text = re.sub(d, "", text)
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = re.sub(r";.*", "", m.group(2))
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        body = re.sub(r"\.Lpost_getpc\d+", ".Lpost_getpc", body)
        out[m.group(1)] = [l.rstrip() for l in body.splitlines() if l.strip()]
    return out


def main(argv):
    drops, rest = [], []
    it = iter(argv)
    for a in it:
        if a == "--drop":
            drops.append(next(it))
        else:
            rest.append(a)
    if len(rest) < 2:
        sys.exit(__doc__)
    old, new = functions(rest[0], []), functions(rest[1], drops)
    out = open(rest[2], "w") if len(rest) > 2 else sys.stdout
    total = differing = 0
    for name, a in old.items():
        b = new.get(name)
        d = -1 if b is None else sum(1 for l in difflib.unified_diff(a, b, lineterm="", n=0) if l[:1] in "+-" and not l.startswith(("---", "+++")))
        total += len(a)
        differing += d != 0
        print("%7d lines %6s differ  %s" % (len(a), "absent" if d < 0 else d, name), file=out)
    for name in new:
        if name not in old:
            print("%7d lines   only new  %s" % (len(new[name]), name), file=out)
    print("%d functions of the older build, %d instruction lines compared, %d functions differ" % (len(old), total, differing), file=out)
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
