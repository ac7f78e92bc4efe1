#!/usr/bin/env python3
"""A/B protocol of the live-row launch -> profiles/r17_live_rows.json.

usage: python tools/profile/live_rows_ab.py --parent DIR --out FILE PHASE [PHASE ...]

DIR is a checkout of the parent commit with its default library built; "new" is this tree.  Every bench / rocprofv3 run is a child
process with its own time limit, one at a time; the first one that fails ends the script (nothing more is started on the GPU).
FILE is read, extended and rewritten after every phase, so the phases can run in separate calls.

  headline   python bench.py --workload W --steps 10 --warmup 3, parent and new alternately, five runs each (ms_per_step)
  trace      rocprofv3 --kernel-trace --stats -- python bench.py --workload W --steps 2 --warmup 1, three runs per build,
             alternating: mean / min / max duration of every kernel
  outputs    bench.py --workload W --steps 2 --warmup 1 --dump-outputs DIR of both builds, compared byte for byte
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
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WORKLOADS = ("t1124", "s1500", "c5share")


def run(cmd, cwd, env=None, limit=300):
    e = dict(os.environ)
    e.pop("PACKPPI_LIB", None)
    e.update(env or {})
    t0 = time.time()
    r = subprocess.run(cmd, cwd=cwd, env=e, capture_output=True, text=True, timeout=limit)
    print(f"[{time.time() - t0:6.1f} s] rc={r.returncode} {os.path.basename(cwd)}: {' '.join(cmd[-8:])}", flush=True)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-3000:], flush=True)
        raise SystemExit(f"child failed ({r.returncode}): nothing more is started")
    return r.stdout


def bench_line(stdout):
    for ln in reversed(stdout.splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("bench.py printed no result line")


def bench(cwd, workload, steps, warmup, env=None, extra=()):
    return bench_line(run([sys.executable, "bench.py", "--gpus", "1", "--workload", workload, "--steps", str(steps), "--warmup",
                           str(warmup), *extra], cwd, env))


def summary(xs):
    return {"runs": [round(x, 4) for x in xs], "mean": round(sum(xs) / len(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def phase_headline(builds, rec):
    out = rec.setdefault("headline_ab", {"command": "python bench.py --gpus 1 --workload W --steps 10 --warmup 3, parent and new "
                                                    "alternately, five runs each (ms_per_step: one pass = context + 100 evaluations)"})
    for w in WORKLOADS:
        ms = {k: [] for k in builds}
        for _ in range(5):
            for k, cwd in builds.items():
                ms[k].append(bench(cwd, w, 10, 3)["ms_per_step"])
        p, n = summary(ms["parent"]), summary(ms["new"])
        out[w] = {"parent": p, "new": n, "ranges_overlap": not (n["max"] < p["min"] or p["max"] < n["min"]),
                  "mean_gain_pct": round(100 * (1 - n["mean"] / p["mean"]), 2),
                  "new_mean_minus_parent_mean": round(n["mean"] - p["mean"], 4), "parent_range_width": round(p["max"] - p["min"], 4)}
        print(w, json.dumps(out[w]), flush=True)


def kernel_stats(cwd, workload):
    d = tempfile.mkdtemp(prefix="live_rows_trace_")
    try:
        run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, "bench.py", "--gpus", "1",
             "--workload", workload, "--steps", "2", "--warmup", "1"], cwd, limit=420)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        rows = {}
        for r in csv.DictReader(open(files[0])):
            rows[r["Name"]] = {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                               "max_us": float(r["MaxNs"]) / 1e3, "total_us": float(r["TotalDurationNs"]) / 1e3}
        return rows
    finally:
        shutil.rmtree(d, ignore_errors=True)


def phase_trace(builds, rec):
    out = rec.setdefault("kernel_trace", {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 "
                                                     "--workload W --steps 2 --warmup 1 (a run of its own; three runs per build, alternating; "
                                                     "per kernel the mean / min / max duration per launch in us of every run, and its share of "
                                                     "the traced kernel time)"})
    for w in WORKLOADS:
        acc = {k: {} for k in builds}
        for _ in range(3):
            for k, cwd in builds.items():
                rows = kernel_stats(cwd, w)
                tot = sum(v["total_us"] for v in rows.values())
                for name, v in rows.items():
                    if not name.startswith(("void k_edge_update", "void k_node_update", "void k_node_message", "k_live_rows")):
                        continue
                    a = acc[k].setdefault(name, {"calls": v["calls"], "mean_us": [], "min_us": [], "max_us": [], "share_of_kernel_time": []})
                    for f in ("mean_us", "min_us", "max_us"):
                        a[f].append(round(v[f], 2))
                    a["share_of_kernel_time"].append(round(v["total_us"] / tot, 4))
        out[w] = acc
        for k in builds:
            for name, a in acc[k].items():
                print(w, k, name[:70], a["calls"], a["mean_us"], a["share_of_kernel_time"], flush=True)


def phase_outputs(builds, rec):
    import numpy as np
    out = rec.setdefault("outputs", {"command": "python bench.py --gpus 1 --workload W --steps 2 --warmup 1 --dump-outputs DIR, parent and "
                                                "new build; the files compared byte for byte"})
    for w in WORKLOADS:
        dirs = {}
        for k, cwd in builds.items():
            dirs[k] = tempfile.mkdtemp(prefix=f"live_rows_out_{k}_")
            bench(cwd, w, 2, 1, extra=("--dump-outputs", dirs[k]))
        names = sorted(os.listdir(dirs["parent"]))
        same = names == sorted(os.listdir(dirs["new"])) and len(names) > 0
        for n in names:
            same = same and open(os.path.join(dirs["parent"], n), "rb").read() == open(os.path.join(dirs["new"], n), "rb").read()
        moved = float(np.abs(np.load(os.path.join(dirs["new"], names[0]))).max()) if names else 0.0
        out[w] = {"files": names, "result": "ALL_EQUAL" if same else "DIFFERENT", "max_abs_of_first_array": moved}
        print(w, out[w], flush=True)
        for d in dirs.values():
            shutil.rmtree(d, ignore_errors=True)
        if not same:
            raise SystemExit("outputs differ")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("phases", nargs="+", choices=["headline", "trace", "outputs"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    builds = {"parent": os.path.abspath(a.parent), "new": ROOT}
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for ph in a.phases:
        {"headline": phase_headline, "trace": phase_trace, "outputs": phase_outputs}[ph](builds, rec)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
