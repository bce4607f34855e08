#!/usr/bin/env python3
"""Are the kernels of two builds the same gfx950 code?  Compares two directories of assembly listings.

Each directory holds one .s per .hip, made with the Makefile's own compile line for that file (its
EXTRA included) with `-c ... -o x.o` replaced by `-S --cuda-device-only -fuse-cuid=none -o DIR/x.s`
(`make -n -B` prints the lines).  Kernels are paired by symbol across all files of a side, so a kernel
that moved to another translation unit still pairs up.  Per kernel two texts are compared: the
lines from `<symbol>:` to its `.Lfunc_end` without the descriptor, and the `.amdhsa_kernel` descriptor
block (registers, LDS, scratch).  Comments are stripped and the function's index within its file is
taken out of local labels (.LBB<n>_<m>, .Lfunc_end<n>, .LJTI<n>_<m>; labels numbered per file, such as
.Ltmp<k>, are renumbered in order of appearance).  Text only: no instruction is looked for.  Prints
one line per kernel that differs with the first differing line pair, lists kernels present on one
side only, and exits 1 on either.  Usage: python tools/isa_same.py PARENT_DIR AFTER_DIR"""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")


def normalise(lines):
    """Comment-free, label-normalised lines of one kernel."""
    seen = {}

    def sub(m):
        name, num, rest = m.group(1), m.group(2), m.group(3)
        if rest is not None or name.startswith("func_"):
            return ".L%sN%s" % (name, rest or "")          # num is the function's index in its file
        return ".L%s#%d" % (name, seen.setdefault((name, num), len(seen)))

    out = []
    for ln in lines:
        ln = LABEL.sub(sub, ln.split(";", 1)[0]).strip()
        if ln:
            out.append(re.sub(r"\s+", " ", ln))
    return out


def kernels_of(text):
    """{symbol: (code lines, descriptor lines)} of one .s text."""
    lines = text.splitlines()
    found = {}
    for ln in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if m and not m.group(1).startswith("__hip_cuid_"):
            found[m.group(1)] = None
    for i, ln in enumerate(lines):
        sym = ln.split(":", 1)[0]
        if ":" not in ln or sym not in found or found[sym] is not None:
            continue
        end = next(k for k in range(i + 1, len(lines)) if lines[k].startswith(".Lfunc_end"))
        body = lines[i:end + 1]
        d0 = next(k for k, x in enumerate(body) if re.match(r"\s*\.amdhsa_kernel\s", x))
        d1 = next(k for k, x in enumerate(body) if re.match(r"\s*\.end_amdhsa_kernel", x))
        found[sym] = (normalise(body[:d0] + body[d1 + 1:]), normalise(body[d0:d1 + 1]))
    return {s: v for s, v in found.items() if v is not None}


def load_dir(path):
    """{symbol: (file name, code, descriptor)} over every .s of a directory."""
    out = {}
    for f in sorted(glob.glob(os.path.join(path, "*.s"))):
        for sym, (code, desc) in kernels_of(open(f).read()).items():
            out[sym] = (os.path.basename(f), code, desc)
    return out


def first_diff(a, b):
    for k in range(max(len(a), len(b))):
        x = a[k] if k < len(a) else "<end>"
        y = b[k] if k < len(b) else "<end>"
        if x != y:
            return k, x, y
    return None


def compare(parent, after):
    """Report lines for two load_dir() results; empty when every kernel is the same."""
    report = []
    for sym in sorted(set(parent) - set(after)):
        report.append("ONLY IN PARENT %s (%s)" % (sym, parent[sym][0]))
    for sym in sorted(set(after) - set(parent)):
        report.append("ONLY AFTER %s (%s)" % (sym, after[sym][0]))
    for sym in sorted(set(parent) & set(after)):
        fa, ca, da = parent[sym]
        fb, cb, db = after[sym]
        for what, d in (("code", first_diff(ca, cb)), ("descriptor", first_diff(da, db))):
            if d:
                report.append("DIFFERS %s (%s -> %s) %s line %d: '%s' | '%s'" % (sym, fa, fb, what, d[0] + 1, d[1], d[2]))
    return report


def main():
    parent, after = load_dir(sys.argv[1]), load_dir(sys.argv[2])
    report = compare(parent, after)
    for ln in report:
        print(ln)
    print("%d kernels at the parent, %d after, %d in both; %d report lines"
          % (len(parent), len(after), len(set(parent) & set(after)), len(report)))
    return 1 if report else 0


if __name__ == "__main__":
    sys.exit(main())
