"""Kernel-by-kernel comparison of gfx950 assembly listings: is every kernel of one build the same
machine code in another (e.g. before and after a source file is split or a switch retired)?
The listings come from
  hipcc <library CFLAGS> <per-file flags> --cuda-device-only -S \\
      -Rpass-analysis=kernel-resource-usage csrc/FILE.hip -o FILE.s 2> FILE.remarks

  python tools/isa_compare.py --old a.s [a.remarks] --new b.s c.s ... [b.remarks c.remarks ...]

Per kernel symbol it compares the instruction stream, the .amdhsa_* directives and the metadata
entry, after normalising what depends only on the position in a file (.LBB<n>_ / .Lfunc_end<n>
labels and the file:line of a remark); each kernel must be in exactly one new listing.  Prints
the counts and exits non-zero on any difference.
"""
import re
import sys


def norm(text):
    text = re.sub(r"\.LBB\d+_", ".LBB_", text)
    text = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", text)
    return re.sub(r"\.Ltmp\d+", ".Ltmp", text)


def kernels(path):
    """{kernel name: (body with its .amdhsa_kernel block, metadata entry)} of a listing."""
    lines = open(path).read().split("\n")
    names = [m.group(1) for m in (re.match(r"\s+\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m]
    body, meta = {}, {}
    i = 0
    while i < len(lines):
        l = lines[i]
        m = re.match(r"^(\S+):", l)
        if m and m.group(1) in names and m.group(1) not in body:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            code = [x.split(";")[0].rstrip() for x in lines[i:j]]
            body[m.group(1)] = norm("\n".join(x for x in code if x))
            i = j
        if re.match(r"  - \.", l):  # a kernel's entry of amdhsa.kernels
            j = i + 1
            while j < len(lines) and lines[j].startswith("   "):
                j += 1
            ent = "\n".join(lines[i:j])
            m = re.search(r"^    \.name:\s+(\S+)", ent, re.M)
            if m:
                meta[m.group(1)] = ent
            i = j - 1
        i += 1
    return {n: (body.get(n), meta.get(n)) for n in names}


def remarks(path):
    """{function name: [resource lines]} of a -Rpass-analysis=kernel-resource-usage log."""
    out, cur = {}, None
    for l in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis", l)
        if not m:
            continue
        f = re.match(r"Function Name: (\S+)", m.group(1))
        if f:
            cur = out.setdefault(f.group(1), [])
        elif cur is not None:
            cur.append(m.group(1))
    return out


def main():
    a = sys.argv[1:]
    old, new = a[a.index("--old") + 1:a.index("--new")], a[a.index("--new") + 1:]
    ko, ro, kn, rn, where = {}, {}, {}, {}, {}
    for p in old:
        (ro if p.endswith(".remarks") else ko).update(remarks(p) if p.endswith(".remarks")
                                                      else kernels(p))
    dup = []
    for p in new:
        if p.endswith(".remarks"):
            rn.update(remarks(p))
            continue
        for n, k in kernels(p).items():
            if n in kn:
                dup.append(n)
            kn[n] = k
            where[n] = p
    missing, extra = sorted(set(ko) - set(kn)), sorted(set(kn) - set(ko))
    differ = [n for n in sorted(set(ko) & set(kn)) if ko[n] != kn[n] or None in ko[n]]
    print("kernels in the old listing          %d" % len(ko))
    print("kernels in the new listings         %d (%s)" % (
        len(kn), ", ".join("%s %d" % (p, sum(1 for w in where.values() if w == p))
                           for p in new if not p.endswith(".remarks"))))
    print("kernels missing / extra / in two    %d / %d / %d" % (len(missing), len(extra), len(dup)))
    print("kernels compared                    %d" % len(set(ko) & set(kn)))
    print("kernels differing                   %d" % len(differ))
    for n in (missing + extra + dup + differ)[:20]:
        print("   ", n)
    bad = len(missing) + len(extra) + len(dup) + len(differ)
    if ro or rn:
        lo = sum(len(v) for v in ro.values())
        dl = sum(1 for n in ro for i, x in enumerate(ro[n])
                 if n not in rn or i >= len(rn[n]) or rn[n][i] != x)
        dl += sum(len(v) for n, v in rn.items() if n not in ro)
        print("resource-usage lines compared       %d (%d functions)" % (lo, len(ro)))
        print("resource-usage lines differing      %d" % dl)
        bad += dl
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
