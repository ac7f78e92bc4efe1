"""What the device shell mask and the mutant workflow cost: an alanine scan of T1124's interface, 32 sets.

    python tools/profile/mutate_scan.py [--sets 32] [--reps 7] [--launches 200] [--steps 30] [--out profiles/r09_mutate_scan.json]

Scan.  ONE pp_ctx_shell launch over the packed batch of all sets (738 rows per set), seeds = the sets' mut_mask, radius 10, in CA
mode (the batch's X) and in ATOM mode (atom14 coordinates at the batch's angles), against the host loop it replaces:
``AffinityPrediction.get_local_subgraph`` once per set on the same device tensors (a copy of the CA coordinates to the host and
torch.cdist there, per set).  Also the other regime: every row a seed, ATOM mode, PP_SHELL_OTHER_CHAIN -- the interface of all sets.
A launch takes microseconds, so one timed window holds --launches launches between two HIP events (per-launch time = window /
launches); the host loop is timed with the wall clock around it (it synchronises by copying).  One warm-up window, then --reps
windows: median, min and max.  The masks of the two paths are compared before anything is timed.

End to end.  ``TDiffusionModule.mutate`` for the same sets at n_decoys = 1 (seeded random weights, --steps reverse steps), wall clock
around a device synchronisation, one warm-up and then three runs.
"""
import argparse
import gzip
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from affinity_scan import scan_sets  # noqa: E402
from packppi_amd.affinity import AffinityPrediction  # noqa: E402
from packppi_amd.batch import as_single, pack  # noqa: E402
from packppi_amd.featurize import mutant_model_data  # noqa: E402
from packppi_amd.functional import _ctx_for  # noqa: E402
from packppi_amd.lib import SHELL_MODES, _ptr, _stream, load  # noqa: E402
from packppi_amd.module import TDiffusionModule  # noqa: E402
from packppi_amd.pdb_io import from_pdb_file  # noqa: E402
from packppi_amd.weights import make_random_state_dict  # noqa: E402


def spread(ms):
    ms = sorted(ms)
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def timed_launches(fn, launches, reps):
    """ms per launch: HIP events around ``launches`` back-to-back calls, one warm-up window, then ``reps`` windows."""
    out = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        b.synchronize()
        if rep:
            out.append(a.elapsed_time(b) / launches)
    return spread(out)


def timed_wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return spread(out)


def raw_launcher(ctx, seeds, mode, flags, xyz):
    """pp_ctx_shell itself on prepared buffers (``Context.shell`` adds the conversions of its arguments, small torch kernels)."""
    lib, dev = load(), ctx.plan.device
    sd = (seeds != 0).to(torch.uint8).reshape(-1).contiguous()
    out = torch.empty(ctx.n_rows, dtype=torch.uint8, device=dev)
    cnt = torch.empty(ctx.n_segments, dtype=torch.int32, device=dev)

    def launch():
        if lib.pp_ctx_shell(ctx.handle, _ptr(sd), SHELL_MODES[mode], 10.0, flags, _ptr(xyz), _ptr(out), _ptr(cnt), _stream(dev)):
            raise RuntimeError(lib.pp_last_error().decode())
    return launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mutate_scan.py measures on the MI355X: no HIP device visible")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz"), "rt") as fh, \
            tempfile.NamedTemporaryFile("w", suffix=".pdb") as tmp:
        tmp.write(fh.read())
        tmp.flush()
        prot = from_pdb_file(tmp.name)
    sets = scan_sets(prot, args.sets)
    dev = torch.device("cuda:0")
    singles = [as_single(mutant_model_data(prot, s, log=lambda m: None)).to(dev) for s in sets]
    pb = pack(singles, trim=False)
    ctx = _ctx_for(pb)
    n_rows, rows_per_set = int(pb.max_size), int(singles[0].max_size)
    seeds = pb.mut_mask
    xyz = ctx.atom14(pb.SC_D)
    every = torch.ones_like(seeds)

    def host_loop():
        return torch.cat([AffinityPrediction.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"]).reshape(-1) for b in singles])

    same = bool(torch.equal(ctx.shell(seeds, 10.0, "ca").reshape(-1).float(), host_loop()))
    ca_shell, ca_count = ctx.shell(seeds, 10.0, "ca", want_count=True)
    atom_shell = ctx.shell(seeds, 10.0, "atom", xyz=xyz)
    iface = ctx.shell(every, 10.0, "atom", other_chain=True, xyz=xyz)
    res = {"workload": f"T1124 fixture, {len(sets)} single-mutation sets X->A, {rows_per_set} rows per set, {n_rows} packed rows, radius 10",
           "device": torch.cuda.get_device_name(0), "build_id": load().pp_build_id().decode(), "reps": args.reps,
           "launches_per_window": args.launches,
           "device_ca_mask_equals_host_loop": same,
           "shell_rows_per_set": {"ca_mean": float(ca_count.float().mean()), "atom_mean": float(atom_shell.sum()) / len(sets),
                                  "interface_mean": float(iface.sum()) / len(sets)},
           "pp_ctx_shell_ca_one_launch_all_sets": timed_launches(raw_launcher(ctx, seeds, "ca", 0, None), args.launches, args.reps),
           "pp_ctx_shell_atom_one_launch_all_sets": timed_launches(raw_launcher(ctx, seeds, "atom", 0, xyz), args.launches, args.reps),
           "pp_ctx_shell_atom_other_chain_every_row_a_seed": timed_launches(raw_launcher(ctx, every, "atom", 1, xyz),
                                                                            max(1, args.launches // 10), args.reps),
           "context_shell_call_ca_with_argument_conversions": timed_launches(lambda: ctx.shell(seeds, 10.0, "ca"), args.launches,
                                                                             args.reps),
           "host_get_local_subgraph_loop_all_sets": timed_wall(host_loop, args.reps)}
    res["host_loop_over_device_ca_launch"] = (res["host_get_local_subgraph_loop_all_sets"]["median_ms"]
                                              / res["pp_ctx_shell_ca_one_launch_all_sets"]["median_ms"])
    print(json.dumps(res), flush=True)

    model = TDiffusionModule(make_random_state_dict(1), device=dev)
    model.schedule = torch.linspace(1, 0, args.steps + 1)
    pairs = [(prot, s) for s in sets]
    res["mutate_end_to_end_n_decoys_1"] = dict(timed_wall(lambda: model.mutate(pairs, seed=1124, log=lambda m: None), 3),
                                               steps=args.steps, sets=len(sets))
    res["mutate_sets_per_s"] = len(sets) * 1e3 / res["mutate_end_to_end_n_decoys_1"]["median_ms"]
    res["saturated"] = model.saturated()
    print(json.dumps(res["mutate_end_to_end_n_decoys_1"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
