"""What a decoy ensemble costs: ``sample_ensemble(select=None)`` of D decoys in ONE packed pass against D
sequential ``sampling(seed=)`` calls of the SAME build, on the T1124 fixture (739 rows, 738 residues) at 100 diffusion steps, and
``pp_ensemble_reduce`` alone.

    python tools/profile/ensemble.py [--decoys 1 4 16] [--steps 100] [--reps 5] [--out profiles/r16_ensemble.json]

The question is the regime (one complex at a time against a packed batch of its replicas), not a regression: both sides run the
same kernels.  HIP events on the current stream around each side, one warm-up and then --reps repetitions; median, min and max.
The sequential side reuses one prepared context (the batch object is the same in every call) and sets the decoy's key per call, as
a caller looping over ``sampling`` would; the packed side reuses the packed batch's context.  Replication and packing (host) are
timed apart, with the wall clock.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bench import load_t1124  # noqa: E402
from packppi_amd.batch import decoy_key, replicate, unpack  # noqa: E402
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
    ap.add_argument("--decoys", type=int, nargs="+", default=[1, 4, 16])
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = TDiffusionModule(make_random_state_dict(1), device=dev)
    model.schedule = torch.linspace(1, 0, args.steps + 1)
    batch = load_t1124()[0].to(dev)
    rows = int(batch.SC_D.shape[1])
    res = {"workload": f"T1124 fixture ({rows} rows), {args.steps} diffusion steps, seeded noise", "reps": args.reps,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for mode in ("sde", "ode"):
        model.hparams.sample_cfg.mode = mode
        for D in args.decoys:
            t0 = time.perf_counter()
            packed = replicate(batch, D)
            t_replicate = (time.perf_counter() - t0) * 1e3
            solos = []
            for d in range(D):
                s = type(batch)(batch)                 # the same tensors: one cached context serves every call
                s["complex_keys"] = [decoy_key(0, d)]
                solos.append(s)

            def sequential():
                return [model.sampling(s, seed=SEED) for s in solos]

            def ensemble():
                return model.sample_ensemble(batch, D, seed=SEED, select=None, return_all=True)

            def packed_sampling():
                return model.sampling(packed, seed=SEED)

            seq = sequential()
            ens, pb = ensemble()["decoys"]
            # pack() drops trailing rows without a residue: a decoy is compared on the rows it has
            same = all(torch.equal(part, seq[d][:, :part.shape[1]]) for d, part in enumerate(unpack(pb, ens)))
            t_seq = timed(sequential, args.reps)
            t_ens = timed(ensemble, args.reps)
            t_pack = timed(packed_sampling, args.reps)
            chi = packed_sampling()
            ctx = model._context(packed)
            per_res = ctx.clash(chi)
            t_clash = timed(lambda: ctx.clash(chi), args.reps)
            t_red = timed(lambda: ctx.ensemble_reduce(chi, D, per_res=per_res, select="clash"), args.reps)
            case = {"mode": mode, "n_decoys": D, "packed_rows": int(packed.max_size), "decoys_bit_equal_to_sequential": bool(same),
                    "sequential_sampling_calls": t_seq, "sample_ensemble_select_none": t_ens,
                    "sampling_of_the_prepared_packed_batch": t_pack, "clash_at_final_angles": t_clash,
                    "pp_ensemble_reduce_select_clash": t_red, "replicate_host_ms": t_replicate,
                    "per_decoy_ms": {"sequential": t_seq["median_ms"] / D, "ensemble": t_ens["median_ms"] / D},
                    "speedup_per_decoy": t_seq["median_ms"] / t_ens["median_ms"],
                    "residues_per_s": {"sequential": 738 * D * 1e3 / t_seq["median_ms"], "ensemble": 738 * D * 1e3 / t_ens["median_ms"]}}
            print(json.dumps(case), flush=True)
            res["cases"].append(case)
    res["saturated"] = model.saturated()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
