"""What the pinned reverse step costs: pp_sample_partial against pp_sample_seeded at T1124, timed with HIP events.

    python tools/profile/partial_sampling.py [--reps 5] [--steps 100] [--out FILE.json]

One prepared context, --steps reverse steps, both modes.  ``seeded`` = pp_sample_seeded; ``partial`` = pp_sample_partial with an
all-zero mask (every row steps: the new instance doing the old work) and with every second row fixed, in both fix modes.  Each
figure is --reps runs after a warm-up, an event pair on the stream around the one call.  The margin to judge the all-zero case
against is the spread (max - min) of the ``seeded`` repetitions themselves.  No speed-up is expected: fixed rows still pay the network.
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


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"ms": [round(t, 3) for t in ts], "median_ms": sorted(ts)[len(ts) // 2], "min_ms": min(ts), "max_ms": max(ts)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = TDiffusionModule(make_random_state_dict(1), device=dev)
    sched = torch.linspace(1, 0, args.steps + 1)
    b, _, _ = load_t1124()
    b = b.to(dev)
    ctx = model._context(b)
    n = ctx.n_rows
    init = ctx.add_noise(b.SC_D, 1.0, 7)
    masks = {"all_free": torch.zeros(n, dtype=torch.uint8, device=dev),
             "half_fixed": (torch.arange(n, device=dev) % 2).to(torch.uint8)}
    res = {"steps": args.steps, "reps": args.reps, "rows": n, "device": torch.cuda.get_device_name(0)}
    for mode in ("ode", "sde"):
        r = {"seeded": timed(lambda: ctx.sample(init, sched, mode, seed=7), args.reps)}
        r["seeded"]["spread_ms"] = r["seeded"]["max_ms"] - r["seeded"]["min_ms"]
        for mname, fixed in masks.items():
            for fix_mode in ("hold", "renoise"):
                key = f"partial_{mname}_{fix_mode}"
                r[key] = timed(lambda: ctx.sample_partial(init, b.SC_D, fixed, sched, mode, 7, fix_mode), args.reps)
                r[key]["median_minus_seeded_ms"] = r[key]["median_ms"] - r["seeded"]["median_ms"]
        res[mode] = r
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
