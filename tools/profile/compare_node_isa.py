"""Compare the device code of pp_node.hip between two builds, kernel by kernel.

    hipcc <product flags> --cuda-device-only -S pp_node.hip -o old.s      (in the old tree)
    hipcc <product flags> --cuda-device-only -S pp_node.hip -o new.s      (in the new tree)
    python tools/profile/compare_node_isa.py old.s new.s

A kernel is the text between its label and its .Lfunc_end.  Names are compared by what the old build calls them: template
arguments and parameter types a newer build APPENDED (a trailing `false` template flag, a trailing struct parameter) are dropped
from the new names, block labels lose their function ordinal.  Per kernel: identical instructions or not, and VGPRs, AGPRs, SGPRs,
scratch and static LDS of both builds from the kernel descriptors (the node kernels' LDS is dynamic: sizeof(SmemU) / sizeof(Smem) at
launch, unchanged unless those structs change).  New kernels are listed with their figures.  Exit status 1 if a pre-existing
node-update instance differs."""
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:", text, flags=re.S | re.M):
        name, body = m.group(1), m.group(2)
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text, flags=re.S)
        if desc is None:
            continue            # a device function, not a kernel
        fig = {k: int(v) for k, v in re.findall(r"\.amdhsa_(next_free_vgpr|next_free_sgpr|accum_offset|group_segment_fixed_size|"
                                                r"private_segment_fixed_size) (\d+)", desc.group(1))}
        body = "\n".join(ln for ln in body.splitlines() if not ln.lstrip().startswith((";", ".")) or ln.lstrip().startswith(".LBB"))
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        out[name] = (body, fig)
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    # map the new names onto the old ones: try the name itself, then with the appended pieces dropped
    mapped = {}
    for n, v in new.items():
        cands = [n, n.replace("5PPRng5PPPin", "5PPRng")]
        cands.append(re.sub(r"ELb0EEv", "EEv", cands[1], count=1))
        key = next((c for c in cands if c in old), n)
        mapped[key] = v
    same = True
    fig = lambda f: "vgpr %3d agpr-offset %3d sgpr %3d scratch %d lds %d" % (
        f.get("next_free_vgpr", 0), f.get("accum_offset", 0), f.get("next_free_sgpr", 0), f.get("private_segment_fixed_size", 0),
        f.get("group_segment_fixed_size", 0))
    for n in sorted(old):
        if n not in mapped:
            print(f"MISSING in the new build: {n}")
            same = False
            continue
        eq = old[n][0] == mapped[n][0]
        if "k_node_update" in n:
            same &= eq and old[n][1] == mapped[n][1]
        figs = fig(old[n][1]) if old[n][1] == mapped[n][1] else fig(old[n][1]) + "  ->  " + fig(mapped[n][1])
        print(f"{'identical' if eq else 'DIFFERENT'}  {len(old[n][0].splitlines()):5d} lines  {figs}  {n}")
    for n in sorted(set(mapped) - set(old)):
        print(f"new        {len(mapped[n][0].splitlines()):5d} lines  {fig(mapped[n][1])}  {n}")
    print("every pre-existing k_node_update / k_node_update_valu instance: identical instructions and resources" if same
          else "pre-existing node-update instances CHANGED")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
