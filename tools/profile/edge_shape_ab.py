#!/usr/bin/env python3
"""Protocol of the edge launch shapes -> profiles/r20_edge_shape.json.

usage: python tools/profile/edge_shape_ab.py --parent DIR --out FILE PHASE [PHASE ...]

DIR is a checkout of the parent commit with its default library built; "new" is this tree.  Every bench / rocprofv3 run is a child
process with its own time limit, one at a time; the first one that fails ends the script (nothing more is started on the GPU).
FILE is read, extended and rewritten after every phase, so the phases can run in separate calls.

  candidates  this tree's diagnostics library (libpackppi_hip.dbg.so) with the launch-shape switches of a MEASUREMENT build
              (PP_LIVE_PAIRS / PP_LIVE_ORDER: the pair workgroups and the order of the live-row work table; PP_EDGE_MIX: the order of
              the all-rows mixed launch), candidates in turn, three rounds of bench.py --steps 10 --warmup 3, and one kernel trace
              per candidate.  The two PP_LIVE_* switches exist only in the build that was measured; they are gone from the sources.
  order       the same on the dispatch order of the all-rows mixed launches at T1124, five rounds: PP_EDGE_MIX (3: one-row workgroups
              first, 1: pairs first; layer-0 edge update and node message) and, in the measured build only, PP_NM_ORDER (the node
              message's order on its own)
  headline    python bench.py --workload W --steps 10 --warmup 3, parent and new alternately, five runs each (ms_per_step)
  trace       rocprofv3 --kernel-trace --stats -- python bench.py --workload W --steps 2 --warmup 1, parent and new alternately, two runs each
  outputs     bench.py --dump-outputs of both builds: the largest wrapped difference of the returned angles
"""
import argparse
import csv
import glob
import json
import os
import shutil
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import live_rows_ab as ab      # noqa: E402  (run / bench / kernel_stats / summary and the headline and trace phases)

ROOT = ab.ROOT
KERNELS = ("void k_edge_update", "void k_node_update", "void k_node_message", "k_live_rows")
# workload -> {candidate: environment}.  569 live rows at T1124 (256 CUs: 190 pairs + 189 one-row is the rule), 1173 at S1500 (512 + 149)
CANDIDATES = {
    "t1124": {"rule_190_pairs_189_one_row": {},
              "256_pairs_57_one_row": {"PP_LIVE_PAIRS": "256"},
              "285_pairs_0_one_row": {"PP_LIVE_PAIRS": "285"},
              "rule_and_all_rows_L0_pairs_first": {"PP_EDGE_MIX": "1"}},
    "s1500": {"rule_512_pairs_149_one_row": {},
              "587_pairs_0_one_row_same_kernel": {"PP_LIVE_PAIRS": "587"},
              "all_rows_PP_EDGE_LIVE_0": {"PP_EDGE_LIVE": "0"}},
}
# the dispatch order of the all-rows mixed launches (layer-0 edge update, stand-alone node message), re-measured behind the live rows
ORDER = {
    "t1124": {"one_row_first_both": {"PP_EDGE_MIX": "3"},
              "edge_pairs_first": {"PP_EDGE_MIX": "1", "PP_NM_ORDER": "3"},
              "message_pairs_first": {"PP_EDGE_MIX": "3", "PP_NM_ORDER": "1"},
              "pairs_first_both": {"PP_EDGE_MIX": "1"}},
}


def phase_order(builds, rec):
    phase_candidates(builds, rec, ORDER, "all_rows_order", 5)


def phase_candidates(builds, rec, CANDIDATES=CANDIDATES, key="candidates", rounds=3):
    from packppi_amd import build
    dbg = build.diag_variant_path()
    if not os.path.exists(dbg):
        raise SystemExit(f"{dbg} is missing")
    out = rec.setdefault(key, {"command": "PACKPPI_LIB=libpackppi_hip.dbg.so + the candidate's switches, python bench.py --gpus 1 "
                                                   "--workload W --steps 10 --warmup 3, candidates in turn, three rounds (five for the order) (ms_per_step); "
                                                   "then one rocprofv3 --kernel-trace --stats run of bench.py --steps 2 --warmup 1 per "
                                                   "candidate (us per launch: mean, min, max)"})
    for w, cands in CANDIDATES.items():
        ms = {k: [] for k in cands}
        for _ in range(rounds):
            for k, env in cands.items():
                ms[k].append(ab.bench(ROOT, w, 10, 3, env=dict(env, PACKPPI_LIB=dbg))["ms_per_step"])
        out[w] = {k: dict(ab.summary(v), env=cands[k]) for k, v in ms.items()}
        for k in cands:
            print(w, k, json.dumps(out[w][k]), flush=True)
        with open(rec["_path"], "w") as f:
            json.dump({a: b for a, b in rec.items() if a != "_path"}, f, indent=1)
    for w, cands in CANDIDATES.items():
        for k, env in cands.items():
            rows = kernel_stats(ROOT, w, dict(env, PACKPPI_LIB=dbg))
            out[w][k]["kernel_trace_us"] = {n[:120]: [v["calls"], round(v["mean_us"], 2), round(v["min_us"], 2), round(v["max_us"], 2)]
                                            for n, v in rows.items() if n.startswith(KERNELS)}
            for n, v in out[w][k]["kernel_trace_us"].items():
                if "k_edge_update" in n or "k_node_message" in n:
                    print(w, k, n[:90], v, flush=True)


def kernel_stats(cwd, workload, env=None):
    """live_rows_ab.kernel_stats with an environment for the child"""
    d = tempfile.mkdtemp(prefix="edge_shape_trace_")
    try:
        ab.run(["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--", sys.executable, "bench.py", "--gpus", "1",
                "--workload", workload, "--steps", "2", "--warmup", "1"], cwd, env, limit=420)
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        return {r["Name"]: {"calls": int(r["Calls"]), "mean_us": float(r["AverageNs"]) / 1e3, "min_us": float(r["MinNs"]) / 1e3,
                            "max_us": float(r["MaxNs"]) / 1e3, "total_us": float(r["TotalDurationNs"]) / 1e3}
                for r in csv.DictReader(open(files[0]))}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def phase_trace(builds, rec):
    out = rec.setdefault("kernel_trace", {"command": "rocprofv3 --kernel-trace --stats --output-format csv -- python bench.py --gpus 1 "
                                                     "--workload W --steps 2 --warmup 1 (a run of its own; two runs per build, alternating; "
                                                     "per kernel [calls, mean, min, max] us per launch of every run)"})
    for w in ab.WORKLOADS:
        acc = {k: {} for k in builds}
        for _ in range(2):
            for k, cwd in builds.items():
                for n, v in kernel_stats(cwd, w).items():
                    if n.startswith(KERNELS):
                        acc[k].setdefault(n[:120], []).append([v["calls"], round(v["mean_us"], 2), round(v["min_us"], 2), round(v["max_us"], 2)])
        out[w] = acc
        for k in builds:
            for n, v in acc[k].items():
                if "k_edge_update" in n:
                    print(w, k, n[:90], v, flush=True)


def phase_outputs(builds, rec):
    import numpy as np
    out = rec.setdefault("outputs", {"command": "python bench.py --gpus 1 --workload W --steps 2 --warmup 1 --dump-outputs DIR, parent and "
                                                "new build: the largest wrapped |difference| of every array, rad (2e-5 is what the "
                                                "one- and two-row instances are held to against each other)"})
    for w in ab.WORKLOADS:
        dirs = {}
        for k, cwd in builds.items():
            dirs[k] = tempfile.mkdtemp(prefix=f"edge_shape_out_{k}_")
            ab.bench(cwd, w, 2, 1, extra=("--dump-outputs", dirs[k]))
        names = sorted(os.listdir(dirs["parent"]))
        if names != sorted(os.listdir(dirs["new"])) or not names:
            raise SystemExit("the two builds dumped different files")
        worst = {}
        for n in names:
            a, b = np.load(os.path.join(dirs["parent"], n)), np.load(os.path.join(dirs["new"], n))
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            worst[n] = float(np.minimum(d, np.abs(2 * np.pi - d)).max()) if a.shape == b.shape else float("inf")
        out[w] = {"max_wrapped_absdiff_rad": worst, "byte_identical": all(v == 0.0 for v in worst.values())}
        print(w, out[w], flush=True)
        for d in dirs.values():
            shutil.rmtree(d, ignore_errors=True)
        if max(worst.values()) > 2e-5:
            raise SystemExit("outputs differ by more than 2e-5 rad")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", required=True)
    ap.add_argument("--out", required=True)
    ap.add_argument("phases", nargs="+", choices=["candidates", "order", "headline", "trace", "outputs"])
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    os.environ.pop("PACKPPI_LIB", None)
    builds = {"parent": os.path.abspath(a.parent), "new": ROOT}
    rec = json.load(open(a.out)) if os.path.exists(a.out) else {}
    rec["_path"] = a.out
    for ph in a.phases:
        {"candidates": phase_candidates, "order": phase_order, "headline": ab.phase_headline, "trace": phase_trace, "outputs": phase_outputs}[ph](builds, rec)
        with open(a.out, "w") as f:
            json.dump({k: v for k, v in rec.items() if k != "_path"}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
