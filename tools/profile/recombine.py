"""What recombining a decoy ensemble per residue buys and costs: on the T1124 fixture (739 rows, 738
residues) at 100 diffusion steps, D seeded decoys with and without the proximal stage, the decoy ``select="clash"`` keeps against
the structure ``pp_ensemble_recombine`` makes from it in at most 64 sweeps.

    python tools/profile/recombine.py [--decoys 4 8 16] [--steps 100] [--sweeps 64] [--reps 5] [--out profiles/r18_recombine.json]

Per case: the time of ``Context.ensemble_recombine`` (HIP events on the current stream, one warm-up, --reps repetitions; median, min
and max) at --sweeps and at 0 sweeps (the reconstruction, the front pass and the two passes behind), the sweeps used, the rows taken
from another decoy, the mean clash before and after, and ``analyze_samples`` (chi error, accuracy, atom RMSD against the input
structure) of both.  The weights are the seeded random ones unless --ckpt names a checkpoint: with random weights the accuracy
columns say nothing about packing quality, only whether recombination moves them.
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bench import load_t1124  # noqa: E402
from packppi_amd.module import TDiffusionModule  # noqa: E402
from packppi_amd.weights import make_random_state_dict  # noqa: E402

SEED = 1124


def timed(fn, reps):
    """ms per call by HIP events: (median, min, max) of ``reps`` calls after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--decoys", type=int, nargs="+", default=[4, 8, 16])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--sweeps", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.ckpt:
        model = TDiffusionModule.load_from_checkpoint(args.ckpt, map_location=dev, strict=False).eval()
    else:
        model = TDiffusionModule(make_random_state_dict(1), device=dev)
    model.schedule = torch.linspace(1, 0, args.steps + 1)
    cfg = model.hparams.sample_cfg
    clash_kw = dict(vtf=cfg.violation_tolerance_factor, tol=cfg.clash_overlap_tolerance)
    batch = load_t1124()[0].to(dev)
    rows = int(batch.SC_D.shape[1])
    res = {"workload": f"T1124 fixture ({rows} rows), {args.steps} diffusion steps, seeded noise, select=clash, {args.sweeps} sweeps",
           "weights": args.ckpt or "seeded random weights (make_random_state_dict(1))", "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "cases": []}

    def metrics(chi):
        m = chi.shape[1]
        full = torch.cat([chi, batch.SC_D[:, m:]], 1) if m != rows else chi      # pack() drops trailing rows without a residue
        return {k: float(v) for k, v in model.analyze_samples(batch, full).items() if k.endswith(("ae_deg", "acc", "rmsd"))}

    for use_proximal in (False, True):
        for D in args.decoys:
            out = model.sample_ensemble(batch, D, seed=SEED, use_proximal=use_proximal, select="clash", return_all=True,
                                        recombine=True, recombine_sweeps=args.sweeps)
            chi, packed = out["decoys"]
            ctx = model._context(packed)
            best = int(out["best"][0])
            t_rec = timed(lambda: ctx.ensemble_recombine(chi, D, start=out["best"], max_sweeps=args.sweeps, **clash_kw), args.reps)
            t_zero = timed(lambda: ctx.ensemble_recombine(chi, D, start=out["best"], max_sweeps=0, **clash_kw), args.reps)
            t_clash = timed(lambda: ctx.clash(chi, cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance), args.reps)
            trace = out["clash_trace"][0].cpu().tolist()
            sweeps = int(out["sweeps"][0])
            case = {"use_proximal": use_proximal, "n_decoys": D, "packed_rows": int(packed.max_size), "best_decoy": best,
                    "recombine": t_rec, "recombine_0_sweeps": t_zero, "pp_clash_of_the_ensemble": t_clash,
                    "ms_per_sweep_used": (t_rec["median_ms"] - t_zero["median_ms"]) / max(sweeps, 1),
                    "sweeps_used": sweeps, "converged": int(out["converged"][0]),
                    "rows_from_another_decoy": int((out["pick"] != best).sum()), "rows": int(out["pick"].numel()),
                    "mean_clash_best_decoy": float(out["clash"][best]), "mean_clash_trace_0": trace[0], "mean_clash_recombined": trace[-1],
                    "metrics_best_decoy": metrics(out["selected"]), "metrics_recombined": metrics(out["recombined"])}
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    res["saturated"] = model.saturated()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
