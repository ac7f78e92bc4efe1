#!/usr/bin/env python3
"""Every host path into the sampler, on small synthetic complexes, as one sha256 per path.

usage: python tools/profile/sampler_paths.py [--out FILE] [--dump FILE.pt]

The weights of ``make_random_state_dict(1)``; synthetic complexes of 33, 40 and 48 rows packed (the shortest that pack, K = 32), one
of 36 rows whose last two are padding (``pack`` trims them, the drivers pad them back) and one of 20 rows, which must go alone.
``model.schedule = linspace(1, 0, 7)`` (six steps: a guide has a first, interior and last nudge point), three proximal steps, two
decoys, four recombination sweeps.  ``compute()`` returns {path: {name: tensor}}; ``digests()`` the sha256 of each path's tensors
(dtype, shape and bytes, in order).  tests/test_sampler_paths.py compares them with tests/golden/r22_sampler_paths.json, recorded
on the commit in front of the host refactor.  --out writes the digests with the library's build id, --dump the tensors themselves.
"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SEED = 1124
GUIDE = dict(scale=0.02, kind="constant")
N_DECOYS, SWEEPS = 2, 4
ENSEMBLE_KEYS = ("selected", "best", "dev", "clash", "consensus", "confidence", "recombined", "pick", "clash_trace", "sweeps",
                 "converged", "bsa")


def _ensemble(out):
    import torch
    res = {k: out[k] for k in ENSEMBLE_KEYS}
    res["decoys"] = out["decoys"][0]
    res["keys"] = torch.tensor([k & 0x7FFFFFFFFFFFFFFF for k in out["keys"]], dtype=torch.int64)
    return res


def _mutation(protein, row, to):
    """One mutation dict (``featurize.parse_mutstr``'s layout) of ``row`` of a synthetic protein to residue type ``to``."""
    from packppi_amd import constants as rc
    return {"wt": rc.restypes[int(protein["aaindex"][row])], "chain": str(protein["chain_id"][row]),
            "resseq": int(protein["residue_index"][row]), "mt": to}


def compute(dev="cuda:0"):
    import torch
    from packppi_amd import synth
    from packppi_amd.batch import pack
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.parallel import sample_sharded
    from packppi_amd.weights import make_random_state_dict

    model = TDiffusionModule(make_random_state_dict(1), device=dev)
    model.schedule = torch.linspace(1, 0, 7)
    cfg = model.hparams.sample_cfg
    cfg.num_steps = 3
    proteins = {n: synth.make_complex(n, 70 + n) for n in (33, 40, 48, 36, 20)}
    cx = {n: protein_to_batch(p).to(dev) for n, p in proteins.items()}
    cx[36]["residue_mask"][:, -2:] = 0                 # trailing padding: pack() drops the rows, the drivers put them back
    for n, c in cx.items():
        c["complex_key"] = 1000 + n
        c["complex_keys"] = [1000 + n]

    def packed():
        return pack([cx[33], cx[40], cx[48]])

    def mask(n):
        return (torch.arange(n, device=dev) % 3 != 0).reshape(1, n)

    out = {}
    for mode in ("ode", "sde"):
        cfg.mode = mode
        torch.manual_seed(0)
        out[f"unseeded_{mode}"] = dict(alone=model.sampling(cx[20]), packed=model.sampling(packed()))
        out[f"seeded_{mode}"] = dict(alone20=model.sampling(cx[20], seed=SEED), alone48=model.sampling(cx[48], seed=SEED),
                                     packed=model.sampling(packed(), seed=SEED))
    cfg.mode = "ode"
    pb = packed()
    fx = mask(pb.max_size)
    for fm in ("hold", "renoise"):
        chi, traj = model.sampling(pb, seed=SEED, fixed_mask=fx, fixed_mode=fm, return_trajectory=True)
        out[f"pinned_{fm}"] = dict(chi=chi, traj=traj)
    chi, traj, trace = model.sampling(pb, seed=SEED, guide=GUIDE, return_trajectory=True)
    out["guided_free"] = dict(chi=chi, traj=traj, trace=trace)
    chi, traj, trace = model.sampling(pb, seed=SEED, guide=GUIDE, fixed_mask=fx, return_trajectory=True)
    out["guided_pinned"] = dict(chi=chi, traj=traj, trace=trace)
    out["proximal"] = dict(alone=model.sampling(cx[48], use_proximal=True, seed=SEED),
                           packed=model.sampling(pb, use_proximal=True, seed=SEED))
    out["repack_proximal"] = dict(packed=model.repack(pb, fx, seed=SEED, use_proximal=True),
                                  alone=model.repack(cx[40], mask(40), seed=SEED, use_proximal=True))
    kw = dict(recombine=True, recombine_sweeps=SWEEPS, sasa=True, return_all=True)
    out["sample_ensemble"] = _ensemble(model.sample_ensemble([cx[33], cx[40]], N_DECOYS, seed=SEED, **kw))
    out["repack_ensemble"] = _ensemble(model.repack_ensemble([cx[33], cx[40]], [mask(33), mask(40)], n_decoys=N_DECOYS, seed=SEED,
                                                             use_proximal=True, **kw))
    sets = [(proteins[48], [_mutation(proteins[48], 10, "A")]), (proteins[40], [_mutation(proteins[40], 5, "F"),
                                                                                  _mutation(proteins[40], 30, "G")]),
            (proteins[20], [_mutation(proteins[20], 3, "A")], 77)]
    res = model.mutate(sets[:2], seed=SEED, n_decoys=N_DECOYS, recombine=True, recombine_sweeps=SWEEPS, sasa=True,
                       log=lambda m: None)
    res += model.mutate(sets[2:], seed=SEED, n_decoys=N_DECOYS, use_proximal=True, max_rows=64, log=lambda m: None)
    out["mutate"] = {f"{i}.{k}": r[k] for i, r in enumerate(res) for k in sorted(r) if isinstance(r[k], torch.Tensor)}
    ids = (33, 40, 48, 36, 20)
    share = [cx[n] for n in ids]
    out["sharded_seeded"], out["sharded_pinned"] = {}, {}
    for rank in (0, 1):
        chis, ids_all, rows = sample_sharded(model, share, rank=rank, world=2, seed=SEED)
        out["sharded_seeded"].update({f"r{rank}.chi{i}": chis[i] for i in sorted(chis)}, **{f"r{rank}.ids": ids_all, f"r{rank}.rows": rows})
        chis, ids_all, rows = sample_sharded(model, share, rank=rank, world=2, seed=SEED, use_proximal=True,
                                             fixed_masks=[mask(n) for n in ids])
        out["sharded_pinned"].update({f"r{rank}.chi{i}": chis[i] for i in sorted(chis)}, **{f"r{rank}.ids": ids_all, f"r{rank}.rows": rows})
    chis, ids_all, rows = sample_sharded(model, share, world=1, rank=0, seed=SEED, use_proximal=True, max_rows=80)
    out["sharded_seeded"].update({f"w1.chi{i}": chis[i] for i in sorted(chis)}, **{"w1.rows": rows})
    ctx = model._context(pb)
    ctx.set_rng_keys(pb.complex_keys)
    out["sample_from"] = dict(packed=model.sample_from(pb, ctx.add_noise(pb.SC_D, 1.0, SEED)))
    torch.cuda.synchronize()
    return out


def digest(tensors):
    import torch
    h = hashlib.sha256()
    for name, t in tensors.items():
        t = t.detach().cpu().contiguous()
        h.update(f"{name}:{t.dtype}:{tuple(t.shape)};".encode())
        h.update(t.reshape(-1).view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def digests(paths):
    return {k: digest(v) for k, v in paths.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    import torch
    from packppi_amd import lib
    paths = compute()
    doc = dict(pp_build_id=lib.load().pp_build_id().decode(), paths=digests(paths))
    print(json.dumps(doc, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
    if a.dump:
        torch.save({k: {n: t.cpu() for n, t in v.items()} for k, v in paths.items()}, a.dump)


if __name__ == "__main__":
    main()
