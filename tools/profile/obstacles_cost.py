#!/usr/bin/env python3
"""Cost of the obstacle term on T1124 with its 78 ligand atoms -> one JSON line.

usage: python tools/profile/obstacles_cost.py [--obstacles] [--steps 50] [--reps 20] [--pdb tests/golden/T1124_lig.pdb.gz]

The proximal stage alone, on a geometry-only context: the angles are the deposited ones plus seeded N(0, 0.5) noise (clashes to work
on), the same in every run.  Reports the mean duration of the one launch per Adam step (pp_profile_kernel(3): the dispatch's own
begin and end) and the wall time of the whole 50-step call (HIP events around `reps` calls behind 3 warm-up calls).  Without
--obstacles the script uses nothing a tree without obstacle support lacks, so it also runs in a checkout of the parent commit:
tools/profile/obstacles_ab.py runs both and alternates."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.getcwd())          # the tree the script is started in (the parent checkout, or this one)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--obstacles", action="store_true")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pdb", default=os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"))
    a = ap.parse_args()
    import torch
    from packppi_amd import pdb_io
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.functional import _ctx_for
    protein = pdb_io.from_pdb_file(a.pdb)
    b = protein_to_batch(protein, obstacles=pdb_io.obstacle_atoms(a.pdb)) if a.obstacles else protein_to_batch(protein)
    b = b.to("cuda:0")
    g = torch.Generator().manual_seed(19)
    chi = ((b.SC_D.cpu() + 0.5 * torch.randn(b.SC_D.shape, generator=g)) * b.SC_D_mask.cpu()).to("cuda:0")
    ctx = _ctx_for(b)
    run = lambda: ctx.proximal_packed(chi, 12.0, 0.5, 1.0, a.steps)
    for _ in range(3):
        out = run()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        out = run()
    e1.record()
    torch.cuda.synchronize()
    wall = e0.elapsed_time(e1) / a.reps
    ctx.profile_kernel(3)
    run()
    step_ms, launches = ctx.profile_read()
    losses = out[3][0].cpu()
    print(json.dumps(dict(obstacles=int(getattr(ctx, "n_obstacles", 0)), rows=int(b.X.shape[1]), steps=a.steps, reps=a.reps,
                          step_launch_us=round(step_ms * 1e3, 3), launches=launches, call_wall_ms=round(wall, 4),
                          loss_first=float(losses[0]), loss_last=float(losses[-1]))))


if __name__ == "__main__":
    main()
