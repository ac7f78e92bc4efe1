"""Compare the device assembly of two tools/debug/isa_digest.sh output folders kernel by kernel.

    python tools/debug/isa_compare.py BEFORE_DIR AFTER_DIR pp_node pp_api ...

For every translation unit and flag set (def, f32, chk, dbg) and every kernel present in BEFORE: its function body with
basic-block label numbers and comments masked, and its kernel descriptor (.amdhsa_kernel block) verbatim.  Kernels only in
AFTER are listed as new.
"""
import os
import re
import sys


def kernels(path):
    text = open(path).read()
    bodies = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*$(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        body = re.sub(r"\.(LBB\d+_\d+|Ltmp\d+|Lfunc_end\d+)", ".L", m.group(2))
        body = "\n".join(ln.split(";")[0].rstrip() for ln in body.splitlines())
        bodies[m.group(1)] = body
    desc = {m.group(1): m.group(2) for m in re.finditer(r"^\s*\.amdhsa_kernel (\w+)\s*$(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)}
    return bodies, desc


def main():
    before, after, units = sys.argv[1], sys.argv[2], sys.argv[3:]
    for unit in units:
        for tag in ("def", "f32", "chk", "dbg"):
            name = f"{unit}.{tag}.s"
            if not os.path.exists(os.path.join(before, name)):
                continue
            b_body, b_desc = kernels(os.path.join(before, name))
            a_body, a_desc = kernels(os.path.join(after, name))
            print(f"== {unit}.{tag}")
            for k in sorted(b_body):
                print(f"  {'identical' if a_body.get(k) == b_body[k] else 'DIFFERENT'}  {k[:60]}")
            same = sum(a_desc.get(k) == v for k, v in b_desc.items())
            print(f"  {same} of {len(b_desc)} descriptors same")
            for k in sorted(set(a_body) - set(b_body)):
                print(f"  new        {k[:60]}")


if __name__ == "__main__":
    main()
