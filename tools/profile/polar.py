"""pp_polar next to pp_sasa on the same context: the record behind DESIGN.md section 27.

    python tools/profile/polar.py --part device --out profiles/r27_polar.json   # HIP events, --reps repetitions after a warm-up
    python tools/profile/polar.py --part trace --out profiles/r27_polar.json    # rocprofv3 --kernel-trace --stats, a run of its own per context

Two contexts: 1BRS (tests/golden/g0_protein_1BRS.npz, 195 rows) and T1124 (tests/golden/T1124_lig.pdb.gz, its ligands as obstacle atoms,
N and O polar) as 8 decoys at seeded random angles (`batch.replicate`).

device: per context the time of one `Context.polar` call and of one `Context.sasa` call on GIVEN coordinates (no atom14 in either):
device events around a call that is followed by a synchronise.  A call is a memset, two kernels and the torch operations behind them
(`polar`, `unsat`, the output allocations): it is not a kernel time.  trace: the duration of `k_polar_prep` and `k_polar` themselves,
from the profiler's kernel statistics of a child process per context (this process never opens the GPU).  Either part keeps the
other's keys of the JSON file.

Next to the times the tool writes what `k_polar` has to do, counted from shapes with torch, not measured: the rows the pre-filter
keeps per row; the pair tests (own polar atoms x atoms of the kept rows, four rows of 16 lanes per step) and their flops (about 40 per
test: two differences, three dot products, the comparisons and ballots); `hbm_bytes`, what has to cross the memory interface once
(coordinates, classes and antecedents in, the workspace out and in, the four arrays out); `l2_bytes`, what the waves fetch again from
the workspace (32 B per staged atom, 16 B per row of the segment for the filter) -- the workspace is 464 B per row, 2.7 MB for the
larger context, and stays in the L2, so these are L2 reads, not memory reads.  Each has a least time at the data-sheet rate (157.3
TFLOP/s fp32 vector, 8 TB/s memory, 34.5 TB/s aggregate L2).  VERDICT: a resource binds the kernel when its least time is at least
half the kernel's duration (trace part; the call time where there is no trace); otherwise none does, and the time is latency: the
launch and the longest wave."""
import argparse
import csv
import glob
import gzip
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
PEAK_FLOPS, PEAK_HBM, PEAK_L2 = 157.3e12, 8.0e12, 34.5e12
BINDS_FROM = 0.5          # share of the time a resource's least time must reach to be called the bound
FLOP_PER_TEST = 40


def load_t1124():
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, obstacle_atoms
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "T1124_lig.pdb")
        with gzip.open(os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"), "rt") as fh, open(path, "w") as out:
            out.write(fh.read())
        return protein_to_batch(from_pdb_file(path), obstacles=obstacle_atoms(path, log=lambda *_: None))   # carries obstacle_polar


def load_1brs():
    from packppi_amd.featurize import protein_to_batch
    z = np.load(os.path.join(ROOT, "tests", "golden", "g0_protein_1BRS.npz"))
    return protein_to_batch({k[5:]: z[k] for k in z.files if k.startswith("prot.")})


def work(ctx, xyz, reach):
    """What k_polar has to do on this context, from shapes (torch on the device): kept rows, pair tests, flops, bytes."""
    import torch
    cls, _ = ctx.polar_tables()
    pol = (cls != 0).reshape(-1, 14)
    X = xyz.reshape(-1, 14, 3)
    ca = X[:, 1]
    d = (X - ca[:, None]).norm(dim=-1)
    rad = torch.where(pol, d, torch.full_like(d, -1.0)).amax(1)
    offs = ctx.seg_offsets_host
    kept_rows = tests = staged = 0
    for lo, hi in zip(offs[:-1], offs[1:]):
        c, r, p = ca[lo:hi], rad[lo:hi], pol[lo:hi].sum(1)
        has = r >= 0
        keep = (torch.cdist(c, c) <= (r[:, None] + r[None] + reach) * 1.001 + 0.01) & has[:, None] & has[None]
        keep.fill_diagonal_(False)
        k = keep.sum(1)
        kept_rows += int(k.sum())
        steps = (k + 3) // 4
        tests += int((steps * 64 * p).sum())
        staged += int(k.sum()) * 14
    n = X.shape[0]
    seg_rows = sum((hi - lo) ** 2 for lo, hi in zip(offs[:-1], offs[1:]))
    ws = n * (14 * 32 + 16)
    return {"polar_atoms": int(pol.sum()), "kept_rows_per_row": kept_rows / max(1, n), "pair_tests": tests,
            "flops": tests * FLOP_PER_TEST, "hbm_bytes": n * (168 + 14 + 28) + 2 * ws + n * (224 + 112 + 32),
            "l2_bytes": staged * 32 + seg_rows * 16, "workspace_bytes": ws}


def verdict(w, seconds):
    """The least times of the counted work and which of them, if any, binds a duration of ``seconds``."""
    floors = {"flops": w["flops"] / PEAK_FLOPS, "memory": w["hbm_bytes"] / PEAK_HBM, "l2": w["l2_bytes"] / PEAK_L2}
    top = max(floors, key=floors.get)
    share = floors[top] / seconds
    return {"least_time_ms": {k: v * 1e3 for k, v in floors.items()}, "largest": top, "largest_share_of_time": share,
            "bound": top if share >= BINDS_FROM else "none of the three: latency (the launch and the longest wave)"}


def device_part(reps, only=None):
    import torch
    from packppi_amd.batch import replicate
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    dev = torch.device("cuda:0")
    out = {"device": torch.cuda.get_device_name(0), "repetitions": reps, "hb_max": 3.5, "sb_max": 4.0, "sasa_points": 96, "runs": {}}

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
        res = ctx.polar(xyz=xyz)
        polar_ms = timed(lambda: ctx.polar(xyz=xyz))
        counts_ms = timed(lambda: ctx.polar(xyz=xyz, want_partners=False))
        sasa_ms = timed(lambda: ctx.sasa(xyz=xyz))
        w = work(ctx, xyz, 4.0)
        out["runs"][name] = {
            "rows": D * n, "segments": D, "obstacle_atoms": int(ctx.n_obstacles),
            "polar_obstacle_atoms": int(pb.obstacle_polar.sum()) if "obstacle_polar" in pb else 0, "polar_call_ms": polar_ms, "polar_counts_only_ms": counts_ms,
            "sasa_call_ms": sasa_ms, "median_polar_call_ms": float(np.median(polar_ms)), "median_sasa_call_ms": float(np.median(sasa_ms)),
            "seg": res.seg.cpu().tolist(), "work_from_shapes": w,
            "against_the_call": verdict(w, float(np.median(polar_ms)) * 1e-3)}
        print(f"{name}: {D * n} rows, polar {np.median(polar_ms):.3f} ms, sasa {np.median(sasa_ms):.3f} ms, "
              f"{json.dumps(out['runs'][name]['against_the_call'])}", flush=True)
    return out


def trace_part(rec, reps):
    """Kernel durations of the two kernels per context, each from a child process of its own under the profiler."""
    out = {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python tools/profile/polar.py --part device --only NAME",
           "runs": {}}
    for name in ("1BRS", "T1124_x8"):
        d = tempfile.mkdtemp(prefix="polar_trace_")
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
                if "k_polar" in r["Name"] or "k_sasa" in r["Name"]:
                    key = r["Name"].split("(")[0].replace("void ", "").strip()
                    rows[key] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                                 "max_us": float(r["MaxNs"]) / 1e3}
        finally:
            shutil.rmtree(d, ignore_errors=True)
        entry = {"kernels": rows}
        main_kernel = [v for k, v in rows.items() if k.startswith("k_polar") and not k.startswith("k_polar_prep")]
        w = rec.get("device_part", {}).get("runs", {}).get(name, {}).get("work_from_shapes")
        if w and main_kernel:
            entry["k_polar_against_its_duration"] = verdict(w, main_kernel[0]["mean_us"] * 1e-6)
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
