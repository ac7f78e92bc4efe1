#!/usr/bin/env python3
"""Cost and effect of clash-guided sampling -> one JSON document (profiles/r21_guided.json).

usage: python tools/profile/guided_cost.py [--steps 100] [--reps 5] [--out FILE]

(b) T1124 (tests/golden/g4_T1124.npz, bench.py's headline batch and initial angles), --steps ODE steps, seeded random weights:
    the wall time of the whole pass (HIP events, `reps` passes alternated behind one warm-up pass of each) unguided
    (Context.sample), guided with eta all zero, with the `late` preset and with `constant`; the launches of a nudge in situ
    (pp_profile_kernel 4, 5, 6: reconstruction, clash + gradient + step, node embedding; the dispatch's own begin and end) in a
    `constant` pass each; and the yardstick, the fused proximal step on the same rows (pp_profile_kernel 3 on the sampled angles).
(c) T1124 with its ligands (tests/golden/T1124_lig.pdb.gz, --obstacles hetero): the clash against the obstacle atoms, summed over the
    residues, and the mean clash at the sampled angles -- before any proximal stage -- unguided, `late` and `constant`.
"""
import argparse
import gzip
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    from packppi_amd import pdb_io
    from packppi_amd.cli.eval_diffusion import obstacle_share
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.schedule import GUIDE_DEFAULTS, guide_eta
    from packppi_amd.weights import make_random_state_dict
    dev = "cuda:0"
    model = TDiffusionModule(make_random_state_dict(20251003), device=dev)
    sched = torch.linspace(1, 0, a.steps + 1)
    model.schedule = sched
    scale, cap = GUIDE_DEFAULTS["scale"], GUIDE_DEFAULTS["cap"]
    etas = {"zero": np.zeros(a.steps + 1, dtype=np.float32), "late": guide_eta(sched, scale, "late", GUIDE_DEFAULTS["t_on"]),
            "constant": guide_eta(sched, scale, "constant")}

    # ---- (b) cost on T1124 ----------------------------------------------------------------------------------------------------
    b, init, _ = bench.load_t1124()
    b, init = b.to(dev), init.to(dev)
    ctx = model._context(b)
    paths = {"unguided": lambda: ctx.sample(init, sched, "ode", seed=1)}
    for name, eta in etas.items():
        paths["guided_" + name] = (lambda e: lambda: ctx.sample_guided(init, sched, "ode", 1, e, cap=cap))(eta)
    out = {k: f() for k, f in paths.items()}
    torch.cuda.synchronize()
    wall = {k: [] for k in paths}
    for _ in range(a.reps):
        for k, f in paths.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            wall[k].append(e0.elapsed_time(e1))
    doc = {"workload": f"T1124 ({int(b.X.shape[1])} rows), {a.steps} ODE steps, seeded random weights, scale {scale}, cap {cap}",
           "zero_eta_equals_unguided": bool(torch.equal(out["unguided"], out["guided_zero"])),
           "nudges": {k: int((e != 0).sum()) for k, e in etas.items()},
           "pass_wall_ms": {k: {"median": sorted(v)[len(v) // 2], "min": min(v), "all": [round(x, 3) for x in v]} for k, v in wall.items()}}
    launches = {}
    for which, name in ((4, "reconstruction"), (5, "clash_gradient_step"), (6, "node_embedding")):
        ctx.profile_kernel(which)
        paths["guided_constant"]()
        ms, n = ctx.profile_read()
        launches[name] = {"mean_us": round(ms * 1e3, 3), "launches": n}          # profile_read: the mean per launch
    chi = out["unguided"]
    ctx.proximal_packed(chi, 12.0, 0.5, 1.0, 50)
    ctx.profile_kernel(3)
    ctx.proximal_packed(chi, 12.0, 0.5, 1.0, 50)
    ms, n = ctx.profile_read()
    launches["yardstick_fused_proximal_step"] = {"mean_us": round(ms * 1e3, 3), "launches": n}
    doc["nudge_launches"] = launches
    doc["nudge_us"] = round(sum(launches[k]["mean_us"] for k in ("reconstruction", "clash_gradient_step", "node_embedding")), 3)
    doc["yardstick_us"] = round(launches["yardstick_fused_proximal_step"]["mean_us"] + launches["reconstruction"]["mean_us"]
                                + launches["node_embedding"]["mean_us"], 3)
    per_res = {k: float(ctx.clash(v).double().mean()) for k, v in out.items()}
    doc["mean_clash_at_the_sample"] = per_res

    # ---- (c) effect next to the ligands of T1124_lig ------------------------------------------------------------------------------
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "T1124_lig.pdb")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"), "rt") as fh, open(path, "w") as fo:
            fo.write(fh.read())
        protein = pdb_io.from_pdb_file(path, mse_to_met=True)
        lb = protein_to_batch(protein, obstacles=pdb_io.obstacle_atoms(path)).to(dev)
    lig = {}
    for name, guide in (("unguided", None), ("late", dict(kind="late")), ("constant", dict(kind="constant"))):
        chi = model.sampling(lb, seed=7, guide=guide)
        share = obstacle_share(model, lb, chi)
        lig[name] = {"clash_against_obstacles_summed": float(sum(share)), "residues_touching": int(sum(1 for v in share if v > 0)),
                     "mean_clash": float(model._context(lb).clash(chi).double().mean())}
    doc["T1124_lig_obstacles_hetero_before_proximal"] = dict(obstacle_atoms=int(lb.obstacle_xyzr.shape[0]), seed=7, **lig)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
