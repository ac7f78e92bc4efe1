"""What the pin costs the proximal stage: pp_proximal_pinned against pp_proximal_packed at T1124, timed with HIP events.

    python tools/profile/pinned_proximal.py [--reps 5] [--steps 50] [--out profiles/r14_pinned_proximal.json]

One prepared context, --steps Adam steps from the fixture's sampled angles.  ``packed`` = pp_proximal_packed; ``pinned_*`` =
pp_proximal_pinned with an all-zero mask (the same work through the other k_prox_init instance), with every second row fixed, and
with everything but the interface fixed (residues with an atom within 10 A of another chain, from the batch's coordinates).  Each
figure is --reps runs after a warm-up, an event pair on the stream around the one call.  The margin to judge the all-zero case against
is the spread (max - min) of the ``packed`` repetitions themselves.  No speed-up is expected: a fixed row still pays its clash
workgroup at every step ("priced, not built").
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from bench import load_t1124  # noqa: E402
from packppi_amd.functional import _ctx_for  # noqa: E402

VTF, TOL, LAMDA = 12.0, 0.5, 1.0


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


def interface_rows(b, radius=10.0, chunk=64):
    """bool [L]: rows with an existing atom within ``radius`` of an existing atom of another chain (B = 1 batch)."""
    X, am, ch = b["X"][0], b["atom_mask"][0] > 0, b["chain_indices"][0]
    L = X.shape[0]
    flat, ok, owner = X.reshape(-1, 3), am.reshape(-1), ch.repeat_interleave(14)
    out = torch.zeros(L, dtype=torch.bool, device=X.device)
    for r0 in range(0, L, chunk):
        r1 = min(r0 + chunk, L)
        d = torch.cdist(X[r0:r1].reshape(-1, 3), flat)                                  # [(r1 - r0) * 14, L * 14]
        near = (d < radius) & ok[None, :] & am[r0:r1].reshape(-1, 1) & (owner[None, :] != ch[r0:r1].repeat_interleave(14)[:, None])
        out[r0:r1] = near.any(1).reshape(r1 - r0, 14).any(1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    b, _, chi = load_t1124()              # the angles the sampler hands the stage: the reference's 100-step output
    b, chi = b.to(dev), chi.float().to(dev)
    ctx = _ctx_for(b)
    n = ctx.n_rows
    inter = interface_rows(b)
    masks = {"all_free": torch.zeros(n, dtype=torch.uint8, device=dev),
             "half_fixed": (torch.arange(n, device=dev) % 2).to(torch.uint8),
             "interface_only": (~inter).to(torch.uint8)}
    res = {"steps": args.steps, "reps": args.reps, "rows": n, "interface_rows": int(inter.sum()),
           "device": torch.cuda.get_device_name(0)}
    res["packed"] = timed(lambda: ctx.proximal_packed(chi, VTF, TOL, LAMDA, args.steps), args.reps)
    res["packed"]["spread_ms"] = res["packed"]["max_ms"] - res["packed"]["min_ms"]
    for name, fixed in masks.items():
        key = f"pinned_{name}"
        res[key] = timed(lambda: ctx.proximal_packed(chi, VTF, TOL, LAMDA, args.steps, fixed=fixed), args.reps)
        res[key]["median_minus_packed_ms"] = res[key]["median_ms"] - res["packed"]["median_ms"]
        res[key]["moved_rows"] = int(ctx.proximal_packed(chi, VTF, TOL, LAMDA, 1, fixed=fixed, return_moved=True)[4].sum())
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
