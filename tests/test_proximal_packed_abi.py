"""CPU-side checks of the packed proximal entry point: declared in the public header, bound by the Python layer, exported by the
library build_library() builds."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    return set(re.findall(r"\b(pp_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", src, flags=re.S)))


def test_pp_proximal_packed_is_declared_bound_and_exported():
    from packppi_amd.build import build_library
    from packppi_amd.lib import SYMBOLS
    assert "pp_proximal_packed" in _declared()
    assert "pp_proximal_packed" in SYMBOLS
    path = build_library(verbose=False)
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "pp_proximal_packed" and " T " in ln for ln in out.splitlines())


def test_pp_proximal_packed_prototype():
    """Ten arguments, the per-complex row counts a HOST int32 table, the losses one row per complex."""
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "packppi_hip.h")).read(), flags=re.S)
    m = re.search(r"pp_status\s+pp_proximal_packed\s*\((.*?)\);", src, flags=re.S)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 10
    assert args[4].startswith("const int32_t") and "norm_rows" in args[4]
    assert [a.split()[-1].lstrip("*") for a in args[5:9]] == ["chi_traj", "chi_last", "chi_accepted", "losses"]
