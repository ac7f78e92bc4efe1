"""pp_chi_refine next to pp_clashscore and pp_hnet_optimize on the same context: the record behind DESIGN.md section 32.

    python tools/profile/refine.py --part device --out profiles/r32_refine.json   # HIP events, --reps repetitions after a warm-up
    python tools/profile/refine.py --part trace --out profiles/r32_refine.json    # rocprofv3 --kernel-trace --stats, a run of its own per context

The two contexts of tools/profile/hnet.py: 1BRS (195 rows; the angles of its own side chains) and T1124 with its ligands as obstacle
atoms as 8 decoys at seeded random angles.  device: the time of one `Context.refine_allatom` (three rounds, its candidate builders
included: a call is its kernels plus the torch operations behind them, not a kernel time), device events around a call followed by
a synchronise, with `Context.clashscore` and `Context.hbond_optimize` at the same angles beside it.  trace: the durations of the
`k_rf_*` kernels and of the candidate builders from the profiler's kernel statistics of a child process per context (this process
never opens the GPU).  Either part keeps the other's keys of the JSON file.

Next to the times: sweeps per round, rows moved, the energy F and the clashscore (rotatable hydrogens not counted) before and after,
and the mean and largest rotation of a moved row.  These are records of crystal coordinates and of seeded random angles with
untuned step sizes, not claims about packing quality."""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from polar import load_1brs, load_t1124      # noqa: E402  (the same inputs)

KERNELS = ("k_rf_angles", "k_rf_prep", "k_rf_compact", "k_rf_partners", "k_rf_propose", "k_rf_apply", "k_rf_finish_seg", "k_atom14",
           "k_hydrogens", "k_aa_prep", "k_clashscore", "k_hn_propose")


def device_part(reps, only=None):
    import torch
    from packppi_amd.batch import replicate
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "repetitions": reps, "deltas_deg": [16, 8, 4], "max_steps": 3, "max_sweeps": 32,
           "bands": 4, "band": 0.15, "cut": 0.4, "hb_allow": 0.6, "runs": {}}

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

    for name, load, D in (("1BRS", load_1brs, 1), ("T1124_x8", load_t1124, 8)):
        if only not in (None, name):
            continue
        b = load().to(dev)
        n = b.X.shape[1]
        pb = replicate(b, D) if D > 1 else b
        ctx = Context(geometry_plan(dev), pb)
        if D > 1:
            g = torch.Generator().manual_seed(D)
            chi = (((torch.rand(1, D * n, 4, generator=g) * 2 - 1) * np.pi).to(dev) * pb.SC_D_mask).contiguous()
        else:
            chi = pb.SC_D.float().contiguous()
        res = ctx.refine_allatom(chi)
        before, after = ctx.clashscore(chi=chi, want_partners=False), ctx.clashscore(chi=res.chi, want_partners=False)
        times = {"refine_allatom": timed(lambda: ctx.refine_allatom(chi)),
                 "refine_allatom_one_round": timed(lambda: ctx.refine_allatom(chi, deltas_deg=(16,))),
                 "refine_allatom_no_sweep": timed(lambda: ctx.refine_allatom(chi, deltas_deg=(16,), max_sweeps=0)),
                 "clashscore": timed(lambda: ctx.clashscore(chi=chi)), "hbond_optimize": timed(lambda: ctx.hbond_optimize(chi=chi))}
        med = {k: float(np.median(v)) for k, v in times.items()}
        rot = torch.rad2deg(res.rotation.abs().sum(-1).reshape(-1)[res.moved.reshape(-1)])
        out["runs"][name] = {"rows": D * n, "segments": D, "obstacle_atoms": int(ctx.n_obstacles),
                             "movers": int((ctx.refine_allatom(chi, deltas_deg=(16,), max_sweeps=0, want_candidates=True).cand_mask != 0).sum()),
                             "sweeps_per_round": res.sweeps.cpu().tolist(), "converged": res.converged.cpu().tolist(),
                             "rows_moved": int(res.moved.sum()), "F_before": res.F[:, 0].cpu().tolist(), "F_after": res.F[:, 1].cpu().tolist(),
                             "F_per_round": res.trace[:, :, -1].cpu().tolist(),
                             "mean_rotation_deg": float(rot.mean()) if rot.numel() else 0.0,
                             "largest_rotation_deg": float(rot.max()) if rot.numel() else 0.0,
                             "clashscore_before": before.clashscore.cpu().tolist(), "clashscore_after": after.clashscore.cpu().tolist(),
                             "call_ms": times, "median_call_ms": med}
        print(f"{name}: {D * n} rows, moved {int(res.moved.sum())}, F {res.F[:, 0].sum().item()} -> {res.F[:, 1].sum().item()}, clashscore "
              f"{[round(v, 2) for v in before.clashscore.cpu().tolist()]} -> {[round(v, 2) for v in after.clashscore.cpu().tolist()]}, "
              + ", ".join(f"{k} {v:.3f} ms" for k, v in med.items()), flush=True)
    return out


def trace_part(rec, reps):
    """Kernel durations per context, each from a child process of its own under the profiler."""
    out = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/profile/refine.py --part device --only NAME",
           "runs": {}}
    for name in ("1BRS", "T1124_x8"):
        d = tempfile.mkdtemp(prefix="refine_trace_")
        try:
            subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                            os.path.abspath(__file__), "--part", "device", "--only", name, "--reps", str(reps), "--out",
                            os.path.join(d, "events.json")], check=True, timeout=280, cwd=ROOT,
                           env=dict(os.environ, HIP_FORCE_DEV_KERNARG=os.environ.get("HIP_FORCE_DEV_KERNARG", "1")))
            files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
            if not files:
                raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
            rows = {}
            for r in csv.DictReader(open(files[0])):
                key = r["Name"].split("(")[0].replace("void ", "").strip()
                if key.startswith(KERNELS):
                    rows[key] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                 "max_us": float(r["MaxNs"]) / 1e3}
        finally:
            shutil.rmtree(d, ignore_errors=True)
        out["runs"][name] = {"kernels": rows}
        print(name, json.dumps(rows), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("device", "trace"), required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--only", default=None, choices=("1BRS", "T1124_x8"))
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    if a.part == "device":
        rec["device_part"] = device_part(a.reps, a.only)
    else:
        rec["trace_part"] = trace_part(rec, a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
