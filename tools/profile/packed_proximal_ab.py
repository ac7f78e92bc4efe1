"""A/B of the proximal stage of parallel.sample_sharded: one packed pp_proximal_packed call per packed group
(packed_proximal=True) against the per-complex loop of proximal_optimizer calls (packed_proximal=False).

Two workloads of BASELINE configs[4] (complexes built as bench.c5_share builds them): the rank-0 share at 8 ranks (32 complexes)
and all 256 complexes on one GPU.  For each: 100 ODE steps from seeded initial angles (bench.c5_inits), then
  - sample_sharded(use_proximal=True) end to end, packed and per-complex alternated, after a warm-up pass of each, every pass
    ending in a device synchronise (wall clock);
  - the proximal stage alone on the same sampled angles (the packed call on the group vs the per-complex loop with its host
    accept rule), timed the same way;
  - the packed per-step launch in situ (pp_profile_kernel(3): HIP events around every Adam-step launch of one packed call);
  - torch.equal of the two paths' angles, ids and metric rows.
Prints one JSON document (and writes it to the path given with --out).

    python tools/profile/packed_proximal_ab.py --reps 3 --out profiles/r06_packed_proximal_ab.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def _stats(xs):
    xs = sorted(xs)
    return {"median_s": xs[len(xs) // 2], "min_s": xs[0], "all_s": [round(x, 6) for x in xs]}


def run_workload(name, model, share, lens, rank, world, reps, dev):
    import torch
    import bench
    from packppi_amd.batch import pack
    from packppi_amd.functional import _ctx_for, proximal_optimizer, proximal_optimizer_packed
    from packppi_amd.parallel import sample_sharded
    cfg = model.hparams.sample_cfg
    inits = bench.c5_inits(share, 4)
    kw = dict(init_chi=inits, lengths=lens, rank=rank, world=world)

    def path(pp):
        return lambda: sample_sharded(model, share, use_proximal=True, packed_proximal=pp, **kw)

    # end to end, alternated after one warm-up pass of each
    res = {True: None, False: None}
    times = {True: [], False: []}
    for pp in (True, False):
        res[pp] = _timed(path(pp), dev)[1]
    for _ in range(reps):
        for pp in (True, False):
            dt, out = _timed(path(pp), dev)
            times[pp].append(dt)
    (c1, i1, r1), (c2, i2, r2) = res[True], res[False]
    equal = (sorted(c1) == sorted(c2) and all(torch.equal(c1[i], c2[i]) for i in c1) and torch.equal(i1, i2)
             and torch.equal(r1, r2))

    # the proximal stage alone, on the sampled angles of the one packed group (every complex here has >= 32 residues)
    plain, _, _ = sample_sharded(model, share, use_proximal=False, **kw)
    ids = sorted(share)
    pb = pack([share[i] for i in ids])
    offs = pb["seg_offsets_host"]
    x = torch.cat([plain[i][:, :b - a] for i, a, b in zip(ids, offs[:-1], offs[1:])], 1)
    sizes = [int(share[i]["max_size"]) for i in ids]
    args = (cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance, cfg.lamda, cfg.num_steps)

    def packed():
        return proximal_optimizer_packed(pb, x, *args, norm_rows=sizes)[2]

    def loop():
        out = {}
        for i in ids:
            lst, losses = proximal_optimizer(share[i], plain[i], *args)
            out[i] = lst[-1] if losses[-1] < losses[0] else plain[i]
        return out
    prox = {"packed": [], "per_complex": []}
    packed(), loop()
    for _ in range(reps):
        prox["packed"].append(_timed(packed, dev)[0])
        prox["per_complex"].append(_timed(loop, dev)[0])
    a_p, a_l = packed(), loop()
    equal_stage = all(torch.equal(a_p[:, a:b], a_l[i][:, :b - a]) for i, a, b in zip(ids, offs[:-1], offs[1:]))

    # the packed Adam-step launch in situ, and the per-complex one on the first complex for scale
    ctx = _ctx_for(pb)
    ctx.profile_kernel(3)
    packed()
    step_ms, launches = ctx.profile_read()
    solo = _ctx_for(share[ids[0]])
    solo.profile_kernel(3)
    proximal_optimizer(share[ids[0]], plain[ids[0]], *args)
    solo_ms, solo_launches = solo.profile_read()

    sp, sl = _stats(times[True]), _stats(times[False])
    pp_, pl = _stats(prox["packed"]), _stats(prox["per_complex"])
    return {
        "workload": name, "complexes": len(share), "rows_packed": offs[-1], "rank": rank, "world": world,
        "ode_steps": len(model.schedule) - 1, "proximal_steps": cfg.num_steps,
        "sample_sharded_packed_proximal": sp, "sample_sharded_per_complex_proximal": sl,
        "sample_sharded_speedup": sl["median_s"] / sp["median_s"],
        "proximal_stage_packed": pp_, "proximal_stage_per_complex": pl,
        "proximal_stage_speedup": pl["median_s"] / pp_["median_s"],
        "packed_step_launch_ms": step_ms, "packed_step_launches": launches,
        "per_complex_step_launch_ms": solo_ms, "per_complex_step_launches": solo_launches,
        "per_complex_step_launch_rows": sizes[0],
        "angles_ids_rows_equal": bool(equal), "proximal_stage_angles_equal": bool(equal_stage),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--workloads", default="share,all", help="comma list of: share (rank 0 of 8), all (256 complexes, 1 GPU)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import bench
    from packppi_amd import synth
    from packppi_amd.parallel import shard_complexes
    lens = synth.c5_lengths(256)
    wl = args.workloads.split(",")
    need = sorted(set(range(256)) if "all" in wl else set(shard_complexes(lens, 8)[0]))
    proteins = bench.c5_proteins(need, min(16, os.cpu_count() or 1))        # host work first: before the GPU is touched
    import torch
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.weights import make_random_state_dict
    dev = torch.device("cuda:0")
    model = TDiffusionModule(make_random_state_dict(20251003), device=dev)
    model.schedule = torch.linspace(1, 0, 101)
    out = {"tool": "tools/profile/packed_proximal_ab.py", "device": torch.cuda.get_device_name(dev), "reps": args.reps,
           "results": []}
    for w in wl:
        rank, world = (0, 8) if w == "share" else (0, 1)
        _, share = bench.c5_share(rank, world, dev, proteins)
        r = run_workload(w, model, share, lens, rank, world, args.reps, dev)
        out["results"].append(r)
        print(json.dumps(r), flush=True)
        del share
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        json.dump(out, open(args.out, "w"), indent=1)
    ok = all(r["angles_ids_rows_equal"] and r["proximal_stage_angles_equal"] for r in out["results"])
    print(json.dumps({"all_equal": ok}))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
