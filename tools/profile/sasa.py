"""pp_sasa on T1124 (tests/golden/T1124_lig.pdb.gz, with its ligands as obstacle atoms): the record behind DESIGN.md section 20.

    python tools/profile/sasa.py --part device --out profiles/r20_sasa.json      # HIP events, five repetitions after a warm-up
    python tools/profile/sasa.py --part host --out profiles/r20_sasa.json        # the NumPy restatement on one complex (CPU only)

device: `Context.sasa` (P = 96, probe 1.4) on the complex alone and on its 4- and 16-decoy replicates (`batch.replicate`, every decoy
at its own seeded random angles through atom14); the time is that of the whole call -- atom14, k_sasa_rows, k_sasa, k_sasa_seg and
the derived tensors -- and of the three pp_sasa launches alone (coordinates given).  host: tests/test_sasa_host.py `restate` in
float32 on the same complex, the only comparison there is.  Either part updates its keys of the JSON file and keeps the other's."""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def load_complex():
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, obstacle_atoms
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "T1124_lig.pdb")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"), "rt") as fh, open(path, "w") as out:
            out.write(fh.read())
        return protein_to_batch(from_pdb_file(path), obstacles=obstacle_atoms(path, log=lambda *_: None))


def device_part(reps):
    import torch
    from packppi_amd.batch import replicate
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    dev = torch.device("cuda:0")
    b = load_complex().to(dev)
    n = b.X.shape[1]
    out = {"device": torch.cuda.get_device_name(0), "rows": n, "atoms": int((b.atom_mask != 0).sum()),
           "obstacle_atoms": int(b.obstacle_xyzr.shape[0]), "n_points": 96, "probe": 1.4, "repetitions": reps, "runs": {}}

    def timed(fn):
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    for D in (1, 4, 16):
        pb = replicate(b, D)
        ctx = Context(geometry_plan(dev), pb)
        g = torch.Generator().manual_seed(D)
        chi = (((torch.rand(1, D * n, 4, generator=g) * 2 - 1) * np.pi).to(dev) * pb.SC_D_mask).contiguous()
        xyz = ctx.atom14(chi)
        res = ctx.sasa(xyz=xyz)
        seg = res.seg_area.cpu().numpy()
        whole, kernels = timed(lambda: ctx.sasa(chi=chi)), timed(lambda: ctx.sasa(xyz=xyz))
        out["runs"][f"decoys_{D}"] = {
            "rows": D * n, "call_with_atom14_ms": whole, "call_on_given_xyz_ms": kernels,
            "median_call_with_atom14_ms": float(np.median(whole)), "median_call_on_given_xyz_ms": float(np.median(kernels)),
            "bsa_A2_per_decoy": (seg[:, 1] - seg[:, 2]).tolist(), "buried_by_obstacles_A2_per_decoy": (seg[:, 2] - seg[:, 3]).tolist(),
            "interface_rows_decoy0": int(res.interface[0, :n].sum()), "pocket_rows_decoy0": int(res.pocket[0, :n].sum())}
        print(f"D = {D:2d}: {D * n} rows, call {np.median(whole):.3f} ms, on given xyz {np.median(kernels):.3f} ms", flush=True)
    # the deposited structure: what --repack interface:sasa and --repack pocket select
    ctx = Context(geometry_plan(dev), b)
    res = ctx.sasa()
    seg = res.seg_area[0].cpu().tolist()
    out["deposited"] = {"seg_area_A2": seg, "bsa_A2": seg[1] - seg[2], "buried_by_obstacles_A2": seg[2] - seg[3],
                        "interface_rows": int(res.interface.sum()), "pocket_rows": int(res.pocket.sum())}
    return out


def host_part():
    from packppi_amd.analysis import sphere_points
    from tests import test_sasa_host as H
    b = load_complex()
    X, radius, chain = H.arrays(b)
    n = X.shape[0]
    t = time.perf_counter()
    counts = H.restate(X, radius, chain, [0, n], sphere_points(96), 1.4, b.obstacle_xyzr.numpy())
    s = time.perf_counter() - t
    a = H.area_fp64(counts, radius, 1.4, 96).sum(0)
    print(f"NumPy restatement, float32, one complex of {n} rows: {s:.1f} s", flush=True)
    return {"rows": n, "numpy_restatement_fp32_s": s, "seg_area_A2": a.tolist(), "threads": os.cpu_count(),
            "note": "brute force over all atoms of the complex, one row at a time; single process"}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("device", "host"), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--merge", default=None, help="an existing record whose other part is kept (default: --out itself)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    src = a.merge or a.out
    rec = json.load(open(src)) if os.path.exists(src) else {}
    rec["device_part" if a.part == "device" else "host_part"] = device_part(a.reps) if a.part == "device" else host_part()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
