"""pp_hydrogens and pp_clashscore next to pp_polar and pp_sasa on the same context: the record behind DESIGN.md section 29.

    python tools/profile/allatom.py --part device --out profiles/r29_allatom.json   # HIP events, --reps repetitions after a warm-up
    python tools/profile/allatom.py --part trace --out profiles/r29_allatom.json    # rocprofv3 --kernel-trace --stats, a run of its own per context

The two contexts of tools/profile/polar.py: 1BRS (195 rows) and T1124 with its ligands as obstacle atoms as 8 decoys at seeded random
angles.  device: the time of one `Context.hydrogens`, one `Context.clashscore` (given the hydrogens: pp_clashscore alone, and with
them: both entries), one `Context.polar` and one `Context.sasa` call on GIVEN coordinates, device events around a call followed by a
synchronise; a call is its kernels plus the torch operations behind them, not a kernel time.  trace: the durations of `k_hydrogens`,
`k_aa_prep` and `k_clashscore` (and `k_polar`, `k_sasa` beside them) from the profiler's kernel statistics of a child process per
context (this process never opens the GPU).  Either part keeps the other's keys of the JSON file.

Next to the times the tool writes what `k_clashscore` has to do, counted from shapes with torch, not measured, in the form of
tools/profile/polar.py: the rows the pre-filter keeps per row (its own included); the pair tests (own counted atoms x atoms of the
kept rows, two rows of 32 lanes per step) and their flops (about 30 per test: a difference, a dot product, the threshold, the
separation and the comparisons); `hbm_bytes`, what crosses the memory interface once (coordinates, hydrogens, radii and classes in,
the workspace out and in, the four arrays out); `l2_bytes`, what the waves fetch again from the workspace (20 B per staged atom, 16 B
per row of the segment for the filter).  The least times at the data-sheet rates and the VERDICT are polar.py's."""
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
from polar import load_1brs, load_t1124, verdict      # noqa: E402  (the same inputs, the same reading)

FLOP_PER_TEST = 30
KERNELS = ("k_hydrogens", "k_aa_prep", "k_clashscore", "k_polar", "k_sasa")


def work(ctx, res, cut):
    """What k_clashscore has to do on this context, from shapes (torch on the device): kept rows, pair tests, flops, bytes."""
    import torch
    r = res.radius.reshape(-1, 27).clone()
    r[:, 14:] *= res.hmask.reshape(-1, 13) != 0
    counted = r > 0
    pos = torch.cat([res.xyz.reshape(-1, 14, 3), res.hxyz.reshape(-1, 13, 3)], 1)
    ca = pos[:, 1]
    d = (pos - ca[:, None]).norm(dim=-1) + r
    rad = torch.where(counted, d, torch.full_like(d, -1.0)).amax(1)
    offs = ctx.seg_offsets_host
    kept_rows = tests = 0
    for lo, hi in zip(offs[:-1], offs[1:]):
        c, rr, p = ca[lo:hi], rad[lo:hi], counted[lo:hi].sum(1)
        has = rr >= 0
        keep = (torch.cdist(c, c) <= (rr[:, None] + rr[None] - cut) * 1.001 + 0.01) & has[:, None] & has[None]
        keep.fill_diagonal_(True)
        k = (keep & has[:, None]).sum(1)
        kept_rows += int(k.sum())
        tests += int((((k + 1) // 2) * 64 * p).sum())
    n = pos.shape[0]
    seg_rows = sum((hi - lo) ** 2 for lo, hi in zip(offs[:-1], offs[1:]))
    ws = n * (27 * 20 + 16)
    return {"counted_atoms": int(counted.sum()), "kept_rows_per_row": kept_rows / max(1, n), "pair_tests": tests,
            "flops": tests * FLOP_PER_TEST, "hbm_bytes": n * (168 + 156 + 13 + 108 + 27 + 1) + 2 * ws + n * (432 + 216 + 16),
            "l2_bytes": kept_rows * 27 * 20 + seg_rows * 16, "workspace_bytes": ws}


def device_part(reps, only=None):
    import torch
    from packppi_amd.batch import replicate
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "repetitions": reps, "cut": 0.4, "hb_allow": 0.6, "rotatable": "skip", "runs": {}}

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
            xyz = ctx.atom14(chi)
        else:
            xyz = pb.X.contiguous()
        h = ctx.hydrogens(xyz=xyz)
        res = ctx.clashscore(xyz=xyz)
        times = {"hydrogens": timed(lambda: ctx.hydrogens(xyz=xyz)), "clashscore_given_hydrogens": timed(lambda: ctx.clashscore(xyz=xyz, hydrogens=h)),
                 "clashscore": timed(lambda: ctx.clashscore(xyz=xyz)),
                 "clashscore_counts_only": timed(lambda: ctx.clashscore(xyz=xyz, hydrogens=h, want_partners=False)),
                 "polar": timed(lambda: ctx.polar(xyz=xyz)), "sasa": timed(lambda: ctx.sasa(xyz=xyz))}
        w = work(ctx, res, 0.4)
        med = {k: float(np.median(v)) for k, v in times.items()}
        out["runs"][name] = {"rows": D * n, "segments": D, "obstacle_atoms": int(ctx.n_obstacles), "hydrogens_placed": int(res.hmask.sum()),
                             "call_ms": times, "median_call_ms": med, "seg": res.seg.cpu().tolist(),
                             "clashscore": res.clashscore.cpu().tolist(), "work_from_shapes": w,
                             "against_the_call": verdict(w, med["clashscore_given_hydrogens"] * 1e-3)}
        print(f"{name}: {D * n} rows, " + ", ".join(f"{k} {v:.3f} ms" for k, v in med.items()), flush=True)
    return out


def trace_part(rec, reps):
    """Kernel durations per context, each from a child process of its own under the profiler."""
    out = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/profile/allatom.py --part device --only NAME",
           "runs": {}}
    for name in ("1BRS", "T1124_x8"):
        d = tempfile.mkdtemp(prefix="allatom_trace_")
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
        entry = {"kernels": rows}
        w = rec.get("device_part", {}).get("runs", {}).get(name, {}).get("work_from_shapes")
        if w and "k_clashscore" in rows:
            entry["k_clashscore_against_its_duration"] = verdict(w, rows["k_clashscore"]["mean_us"] * 1e-6)
        out["runs"][name] = entry
        print(name, json.dumps(entry), flush=True)
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
