"""SDE sampling with seeded in-kernel noise against the explicit-noise path: time at T1124 and memory of the 256-complex job.

    python tools/profile/seeded_noise.py [--reps 7] [--steps 100] [--skip-c5] [--out FILE.json]

(b) T1124, --steps reverse steps, sde mode, one prepared context: ``seeded`` = add_noise + pp_sample_seeded; ``explicit`` =
pp_sample on a [steps, 2, N, 4] noise tensor made OUTSIDE the timed region; ``sampling_unseeded`` = TDiffusionModule.sampling()
without a seed, its two randn_like and 2 x steps torch.normal calls included.  Median, min and max of --reps runs after a warm-up,
wall clock around a device synchronisation.  On a library without the seeded calls only the last two are measured.
(c) BASELINE configs[4] (256 synthetic complexes, one packed batch, sde): device memory taken outside torch's allocator while the
context lives (the library's arena, from hipMemGetInfo) and the rise of torch's peak across one sampling() call, seeded and unseeded.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bench import c5_proteins, c5_share, load_t1124  # noqa: E402
from packppi_amd.batch import pack  # noqa: E402
from packppi_amd.lib import Context  # noqa: E402
from packppi_amd.module import TDiffusionModule  # noqa: E402
from packppi_amd.weights import make_random_state_dict  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": ts[len(ts) // 2], "min_ms": ts[0], "max_ms": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--skip-c5", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    proteins = None if args.skip_c5 else c5_proteins(range(256), 16)       # host work before the GPU is touched
    has_seeded = hasattr(Context, "sample") and "seed" in Context.sample.__code__.co_varnames
    model = TDiffusionModule(make_random_state_dict(1), sample_cfg=dict(mode="sde"), device=dev)
    model.schedule = torch.linspace(1, 0, args.steps + 1)
    res = {"steps": args.steps, "reps": args.reps, "seeded_calls": has_seeded, "device": torch.cuda.get_device_name(0)}

    b, init, _ = load_t1124()
    b, init = b.to(dev), init.to(dev)
    ctx = model._context(b)
    n = ctx.n_rows
    noise = torch.randn(args.steps, 2, n, 4, device=dev)
    t1124 = {"rows": n}
    t1124["explicit"] = timed(lambda: ctx.sample(init, model.schedule, "sde", sde_noise=noise), args.reps)
    t1124["sampling_unseeded"] = timed(lambda: model.sampling(b), args.reps)
    if has_seeded:
        t1124["seeded"] = timed(lambda: ctx.sample(ctx.add_noise(b.SC_D, 1.0, 7), model.schedule, "sde", seed=7), args.reps)
        t1124["sampling_seeded"] = timed(lambda: model.sampling(b, seed=7), args.reps)
    res["t1124_sde"] = t1124
    del ctx, noise
    model._ctx_key, model._ctx = None, None

    if not args.skip_c5:
        _, share = c5_share(0, 1, dev, proteins)
        pb = pack(list(share.values()))
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        reserved0 = torch.cuda.memory_reserved()
        model._context(pb)
        torch.cuda.synchronize()
        arena = (free0 - torch.cuda.mem_get_info()[0]) - (torch.cuda.memory_reserved() - reserved0)
        c5 = {"rows": int(pb.max_size), "complexes": len(share), "outside_torch_bytes": int(arena),
              "chi_bytes": int(pb.max_size) * 16}
        for name, kw in (("unseeded", {}),) + ((("seeded", {"seed": 7}),) if has_seeded else ()):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            t0 = time.perf_counter()
            model.sampling(pb, **kw)
            torch.cuda.synchronize()
            c5[name] = {"torch_peak_rise_bytes": int(torch.cuda.max_memory_allocated() - base),
                        "wall_ms": (time.perf_counter() - t0) * 1e3}
        res["c5_256_sde"] = c5
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
