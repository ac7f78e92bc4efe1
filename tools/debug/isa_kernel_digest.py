#!/usr/bin/env python3
"""usage: tools/debug/isa_kernel_digest.py A.s [B.s]

Per-kernel digests of a device assembly file written by tools/debug/isa_digest.sh: for every function its demangled name, the
number of instruction lines and a digest of its instructions and labels (directives and comments dropped, the compilation-unit id
and the per-file numbering of local labels masked).  With two files (A = the older tree): a kernel of B whose name is one of A's
with a trailing `, false` template argument appended -- and possibly one more kernel parameter behind the old ones -- counts as that
kernel (a new template parameter whose `false` instances must be the old kernels); which kernels have the same
instructions in both, which differ, which exist in one only -- what a pull request that adds template instances quotes to show
that the existing instances kept theirs (profiles/r17_live_rows.json)."""
import hashlib
import re
import subprocess
import sys


def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*(;.*)?$", ln)
        if name is None and m and not m.group(1).startswith(".L") and m.group(1).startswith("_Z"):
            name, body = m.group(1), []
            continue
        if name is not None:
            if ln.startswith(".Lfunc_end"):
                ins = [b for b in body if b.strip() and not b.lstrip().startswith(";") and not (b.startswith("\t") and b.lstrip().startswith("."))]
                ins = [b.split(";")[0].rstrip() + "\n" for b in ins]          # trailing comments: loop notes padded to the label's width
                text = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid_X", "".join(ins))
                text = re.sub(r"\.LBB\d+_", ".LBB_", text)
                text = re.sub(r"\bBB\d+_", "BB_", text)          # the same numbering in the comments that trail label lines
                n_ins = sum(1 for b in ins if b.startswith("\t"))
                out[name] = (hashlib.sha256(text.encode()).hexdigest()[:16], n_ins)
                name = None
            else:
                body.append(ln)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(argv):
    a = kernels(argv[1])
    if len(argv) < 3:
        d = demangle(sorted(a))
        for n in sorted(a):
            print(f"{a[n][0]}  {a[n][1]:6d}  {d[n]}")
        return 0
    b = kernels(argv[2])
    d = demangle(sorted(set(a) | set(b)))
    a = {d[n]: v for n, v in a.items()}
    b = {d[n]: v for n, v in b.items()}
    for n in list(b):          # a new defaulted template parameter, with or without a new last kernel parameter for it
        old = re.sub(r", false>\(", ">(", n, count=1)
        for cand in (old, re.sub(r", [\w:]+\)$", ")", old)):
            if n not in a and cand in a and cand not in b:
                b[cand] = b.pop(n)
                break
    d = {n: n for n in set(a) | set(b)}
    same = [n for n in a if n in b and a[n] == b[n]]
    diff = [n for n in a if n in b and a[n] != b[n]]
    print(f"{len(same)} kernels with the same instructions, {len(diff)} that differ, {len(set(a) - set(b))} only in {argv[1]}, "
          f"{len(set(b) - set(a))} only in {argv[2]}")
    for n in sorted(diff):
        print(f"DIFFERS   {a[n][0]} {a[n][1]:6d} | {b[n][0]} {b[n][1]:6d}  {d[n]}")
    for n in sorted(set(a) - set(b)):
        print(f"ONLY IN A {a[n][0]} {a[n][1]:6d}  {d[n]}")
    for n in sorted(set(b) - set(a)):
        print(f"ONLY IN B {b[n][0]} {b[n][1]:6d}  {d[n]}")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
