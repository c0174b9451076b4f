#!/usr/bin/env python3
"""Compare the kernels of two assembly listings: kernel_text_diff.py A.s B.s

A listing is what `hipcc <the Makefile's flags> --cuda-device-only -S file.hip -o file.s` writes (several listings concatenated
are one listing: that is how the kernels of a file that was split are held against the file they came from).  For every kernel,
named by its `.amdhsa_kernel` line, two things are compared as text:

  * the instructions: the lines from the kernel's label to its `.Lfunc_end` label, without comments and blank lines, with the
    function number taken out of the local labels (`.LBB<n>_<m>`, `.LJTI<n>_<m>`), which counts the functions of the file and
    so changes when a kernel moves;
  * the resources: the `.amdhsa_` lines of its kernel descriptor (registers, scratch, LDS, ...).

It prints which kernels are only in A, only in B, defined more than once, different, and the same, and exits 1 unless both
listings hold the same kernels, each once, with the same text.  It compares text; it looks for no particular instruction.
"Identical" is about these two things only, not about the objects: what lies outside a kernel's label .. `.Lfunc_end` range and its
descriptor (constants in `.rodata`, jump tables, other functions, metadata) is not compared.
"""
import itertools
import re
import sys

_LOCAL = re.compile(r"\.L(BB|JTI)\d+_")


def _strip(line):
    """One line without its comment and surrounding blanks, local labels normalised."""
    return _LOCAL.sub(r".L\1_", line.split(";", 1)[0].strip())


def kernels(text):
    """{name: [(instructions, resources), ...]} of one listing; a name defined once has one entry."""
    lines = text.splitlines()
    labels = {}
    for i, line in enumerate(lines):
        m = re.match(r"([A-Za-z_$][\w$.]*):", line)
        if m:
            labels.setdefault(m.group(1), []).append(i)
    found = {}
    seen = {}
    for i, line in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        name = m.group(1)
        nth = seen.get(name, 0)
        seen[name] = nth + 1
        res = []
        for r in lines[i + 1:]:
            if r.strip().startswith(".end_amdhsa_kernel"):
                break
            r = _strip(r)
            if r:
                res.append(r)
        body = []
        starts = labels.get(name, [])
        if nth < len(starts):
            for b in lines[starts[nth] + 1:]:
                if re.match(r"\.Lfunc_end\d+:", b):
                    break
                b = _strip(b)
                if b:
                    body.append(b)
        found.setdefault(name, []).append((body, res))
    return found


def compare(text_a, text_b):
    """(report lines, number of findings) for two listings."""
    a, b = kernels(text_a), kernels(text_b)
    out = []
    only_a = sorted(set(a) - set(b))
    only_b = sorted(set(b) - set(a))
    twice = sorted(n for side in (a, b) for n in side if len(side[n]) > 1)
    differ, same = [], []
    for name in sorted(set(a) & set(b)):
        (ia, ra), (ib, rb) = a[name][0], b[name][0]
        what = [w for w, x, y in (("instructions", ia, ib), ("resources", ra, rb)) if x != y]
        if not ia or not ib:
            what.append("no instruction text found")
        if what:
            differ.append((name, what, ra, rb))
        else:
            same.append(name)
    out.append("kernels: %d in A, %d in B" % (len(a), len(b)))
    for title, names in (("only in A", only_a), ("only in B", only_b), ("defined more than once", twice)):
        out.append("%s: %d" % (title, len(names)))
        out.extend("  " + n for n in names)
    out.append("different: %d" % len(differ))
    for name, what, ra, rb in differ:
        out.append("  %s: %s" % (name, ", ".join(what)))
        for x, y in itertools.zip_longest(ra, rb, fillvalue="(no line)"):
            if x != y:
                out.append("    A %s | B %s" % (x, y))
    out.append("same instructions and resources: %d" % len(same))
    out.extend("  " + n for n in same)
    return out, len(only_a) + len(only_b) + len(twice) + len(differ)


def main(argv):
    if len(argv) != 3:
        sys.stderr.write(__doc__)
        return 2
    with open(argv[1]) as fa, open(argv[2]) as fb:
        out, findings = compare(fa.read(), fb.read())
    print("\n".join(out))
    print("RESULT: %s" % ("identical" if findings == 0 else "%d finding(s)" % findings))
    return 0 if findings == 0 else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv))
