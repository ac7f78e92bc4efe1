#!/usr/bin/env python3
"""Cost of predictor-corrector sampling -> one JSON document (profiles/r23_corrector.json).

usage: python tools/profile/corrector_cost.py [--steps 30] [--runs 3] [--out FILE] [--no-trace] [--plain-only]

T1124 (tests/golden/g4_T1124.npz, bench.py's headline batch and initial angles), --steps SDE steps, seeded random weights, one
process: behind one warm-up pass of each, `runs` passes plain (Context.sample(seed=)) and `runs` passes with a corrector behind
every step but the last (Context.sample_corrected, schedule.corrector_snr), alternated, each between two HIP events.  Derived: the
extra time of a corrected step, and that extra less one plain evaluation -- what the corrector launch, the un-fused node embedding
and the launch gaps cost together.  k_correct's own duration comes from one `rocprofv3 --kernel-trace --stats` run of this script
(a child process of its own, --child) and, next to it, from the in-situ event pair (pp_profile_kernel 7).
--plain-only: only the plain series (this is the command that also runs on the parent commit, which has no corrector).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def setup(steps):
    import torch
    import bench
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.weights import make_random_state_dict
    dev = "cuda:0"
    model = TDiffusionModule(make_random_state_dict(20251003), device=dev)
    sched = torch.linspace(1, 0, steps + 1)
    b, init, _ = bench.load_t1124()
    b, init = b.to(dev), init.to(dev)
    return model._context(b), init, sched, int(b.X.shape[1])


def timed(f):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    f()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def series(v):
    return {"median": sorted(v)[len(v) // 2], "min": min(v), "max": max(v), "all": [round(x, 3) for x in v]}


def kernel_trace(steps):
    """k_correct's row of one rocprofv3 --kernel-trace --stats run of `--child` (two corrected passes)."""
    d = tempfile.mkdtemp(prefix="corr_trace_")
    try:
        subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable,
                        os.path.abspath(__file__), "--child", "--steps", str(steps)], cwd=ROOT, check=True, timeout=300,
                       stdout=subprocess.DEVNULL)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        for r in csv.DictReader(open(files[0])):
            if "k_correct" in r["Name"]:
                return {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                        "max_us": float(r["MaxNs"]) / 1e3}
        raise SystemExit("no k_correct row in the kernel trace")
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    import torch
    ctx, init, sched, rows = setup(a.steps)
    plain = lambda: ctx.sample(init, sched, "sde", seed=1)
    if a.plain_only:
        plain()
        torch.cuda.synchronize()
        doc = {"workload": f"T1124 ({rows} rows), {a.steps} SDE steps, seeded random weights", "plain_pass_ms": series([timed(plain) for _ in range(a.runs)])}
    else:
        from packppi_amd.schedule import corrector_snr
        snr = corrector_snr(sched, 0.16)
        corrected = lambda: ctx.sample_corrected(init, sched, "sde", 1, snr)
        if a.child:
            corrected(), corrected()
            torch.cuda.synchronize()
            return
        zero = ctx.sample_corrected(init, sched, "sde", 1, snr * 0)
        same = bool(torch.equal(plain(), zero))
        corrected()
        torch.cuda.synchronize()
        wall = {"plain": [], "corrected": []}
        for _ in range(a.runs):
            wall["plain"].append(timed(plain))
            wall["corrected"].append(timed(corrected))
        n_corr = int((snr != 0).sum())
        p, c = sorted(wall["plain"])[a.runs // 2], sorted(wall["corrected"])[a.runs // 2]
        extra = (c - p) / n_corr
        doc = {"workload": f"T1124 ({rows} rows), {a.steps} SDE steps, seeded random weights, snr 0.16 behind {n_corr} of {a.steps} steps",
               "zero_snr_equals_plain": same,
               "plain_pass_ms": series(wall["plain"]), "corrected_pass_ms": series(wall["corrected"]),
               "plain_step_us": round(p / a.steps * 1e3, 3),
               "extra_per_corrected_step_us": round(extra * 1e3, 3),
               "extra_minus_one_plain_evaluation_us": round((extra - p / a.steps) * 1e3, 3),
               "corrected_over_plain_step": round(1 + extra / (p / a.steps), 3)}
        ctx.profile_kernel(7)
        corrected()
        ms, n = ctx.profile_read()
        doc["k_correct_in_situ"] = {"mean_us": round(ms * 1e3, 3), "launches": n}
        if not a.no_trace:
            doc["k_correct_kernel_trace"] = kernel_trace(a.steps)
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
