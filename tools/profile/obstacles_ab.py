#!/usr/bin/env python3
"""A/B protocol of the obstacle pull request -> profiles/r19_obstacles.json.

usage: python tools/profile/obstacles_ab.py --parent DIR --out FILE [--runs 3] PHASE [PHASE ...]

DIR is a checkout of the parent commit with its default library built; "new" is this tree.  Every run is a child process with its
own time limit, one at a time, parent and new alternately; the first one that fails ends the script (nothing more is started on
the GPU).  FILE is read, extended and rewritten after every phase.

  headline   python bench.py --gpus 1 --steps 10 --warmup 3 (the flagship workload; nothing on its path changes)
  proximal   the same with --proximal (the 50-step proximal stage of a context WITHOUT obstacles: the instances of before)
  cost       tools/profile/obstacles_cost.py: parent, new without obstacles, new with T1124's 78 obstacle atoms
"""
import argparse
import json
import os
import shutil
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(cmd, cwd, limit=240):
    e = dict(os.environ)
    e.pop("PACKPPI_LIB", None)
    t0 = time.time()
    r = subprocess.run(cmd, cwd=cwd, env=e, capture_output=True, text=True, timeout=limit)
    print(f"[{time.time() - t0:6.1f} s] rc={r.returncode} {os.path.basename(cwd)}: {' '.join(cmd[1:])}", flush=True)
    if r.returncode != 0:
        print(r.stdout[-2000:], r.stderr[-3000:], flush=True)
        raise SystemExit(f"child failed ({r.returncode}): nothing more is started")
    for ln in reversed(r.stdout.splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("the child printed no result line")


def summary(xs):
    return {"runs": [round(x, 4) for x in xs], "mean": round(sum(xs) / len(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("phases", nargs="+", choices=("headline", "proximal", "cost"))
    a = ap.parse_args()
    parent = os.path.abspath(a.parent)
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    for ph in a.phases:
        if ph in ("headline", "proximal"):
            cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3"] + (["--proximal"] if ph == "proximal" else [])
            ms = {"parent": [], "new": []}
            for _ in range(a.runs):
                for name, cwd in (("parent", parent), ("new", ROOT)):
                    ms[name].append(float(run(cmd, cwd)["ms_per_step"]))
            rec[ph] = {"command": " ".join(cmd[1:]) + ", parent and new alternately; ms_per_step",
                       "parent": summary(ms["parent"]), "new": summary(ms["new"])}
        else:
            script = os.path.join("tools", "profile", "obstacles_cost.py")
            os.makedirs(os.path.join(parent, "tools", "profile"), exist_ok=True)
            shutil.copy(os.path.join(ROOT, script), os.path.join(parent, script))
            pdb = os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz")
            rows = {"parent": [], "new_without": [], "new_with": []}
            for _ in range(a.runs):
                for name, cwd, extra in (("parent", parent, []), ("new_without", ROOT, []), ("new_with", ROOT, ["--obstacles"])):
                    rows[name].append(run([sys.executable, script, "--pdb", pdb] + extra, cwd))
            rec["cost"] = {"command": "python tools/profile/obstacles_cost.py [--obstacles], alternately",
                           **{k: {"step_launch_us": summary([r["step_launch_us"] for r in v]),
                                  "call_wall_ms": summary([r["call_wall_ms"] for r in v]), "obstacles": v[0]["obstacles"],
                                  "rows": v[0]["rows"], "loss_first": v[0]["loss_first"], "loss_last": v[0]["loss_last"]}
                              for k, v in rows.items()}}
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)
            fh.write("\n")
        print(json.dumps(rec[ph]), flush=True)


if __name__ == "__main__":
    main()
