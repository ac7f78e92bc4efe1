"""Container-only: the UNMODIFIED reference on structures with incomplete side chains -> tests/golden/g13_incomplete_*.npz.

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/make_golden_incomplete.py [--only L40,L97,B2,1BRS] [--threads 8]

Inputs: ``synth.drop_atoms`` on synthetic complexes of 40 and 97 residues, a padded batch of two (40 and 36 rows), and on the
committed protein dict of 1BRS (g0_protein_1BRS, which lacks atoms of its own).  Every damaged dict is featurised by the reference's
``prot_to_data`` and by ``packppi_amd.featurize``; the two must agree, and the dict and the reference's tensors are stored as in g0.
Weights: ``make_random_state_dict(20251003)``, as in every other fixture.

Stored per file (data only): the batch, the reference's neighbour lists and embedded edges (hE0 on ``hE0_rows``: the damaged rows,
the masked row and the numbering gap with their neighbours -- the full tensor would be past the size a committed file may have),
h_V and the score at t = 1, 0.5, 1/30, atom14 at the initial angles, the per-residue clash at (12.0, 0.5) with its autograd
gradient in fp32 and fp64, the 30-step ODE result in fp32 and in fp64 with cond = max |ref32 - ref64|, and five steps of the reference's
``proximal_optimizer`` per complex in both precisions (angles, losses, its clash mask).  L40 also holds the per-layer states.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refshim  # noqa: E402
from make_golden import WEIGHT_SEED, pack_batch, seeded_init  # noqa: E402
from make_golden_prox import ref_batch, wrapped  # noqa: E402
from packppi_amd import synth  # noqa: E402
from packppi_amd.batch import TENSOR_KEYS, as_single, collate, split  # noqa: E402
from packppi_amd.featurize import protein_to_data  # noqa: E402
from packppi_amd.weights import make_random_state_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
INIT_SEED = 13
N_STEPS = 30
PROX_STEPS = 5
HE_ROWS = 24
MAX_BYTES = 1 << 20
PROT_KEYS = ("atom_positions", "atom_mask", "aaindex", "residue_index", "chain_id", "b_factors")


def cases():
    """tag -> list of damaged protein dicts (more than one: a padded batch).  The damage seeds are kept to those under which the
    reference's own fp32 and fp64 proximal runs stay within 1e-6 rad of each other over the five steps (tests/test_incomplete_host.py
    asserts it): Adam divides by the gradient's magnitude, so an entry whose gradient passes through zero is steered by fp32 rounding
    (L97 under damage seed 97: 7.9e-6 rad on one entry with a complete side chain), and such an input cannot arbitrate at 2e-5.
    Likewise every exact zero of the reference's fp32 clash gradient must be a zero of its fp64 gradient too -- an angle no active term
    depends on -- since the GPU test demands exact zeros there: under damage seed 98 one complete ARG of L97 has a chi2 gradient of
    8.1e-10 in fp64 that fp32 happens to cancel to -0.0, which no other summation order reproduces."""
    z = np.load(os.path.join(GOLD, "g0_protein_1BRS.npz"))
    brs = {k: z["prot." + k] for k in PROT_KEYS}
    return {"L40": [synth.drop_atoms(synth.make_complex(40, 1340), 40)],
            "L97": [synth.drop_atoms(synth.make_complex(97, 1397), 100)],
            "B2": [synth.drop_atoms(synth.make_complex(40, 1440), 41), synth.drop_atoms(synth.make_complex(36, 1436), 37)],
            "1BRS": [synth.drop_atoms(brs, 195)]}


def interesting_rows(prots, L, limit):
    """Flat row numbers of the [B, L] batch whose embedded edges are kept: masked rows and numbering gaps with their neighbours
    first, then the damaged rows, then the rest in order."""
    first, second = [], []
    for s, p in enumerate(prots):
        kinds = synth.damage_kinds(p)
        n = len(kinds)
        ridx, chain = np.asarray(p["residue_index"]), np.asarray(p["chain_id"])
        for i in range(n):
            gap = i > 0 and chain[i] == chain[i - 1] and ridx[i] != ridx[i - 1] + 1
            if kinds[i] == "masked" or gap:
                first += [s * L + j for j in range(max(0, i - 2), min(n, i + 3))]
            elif kinds[i] is not None:
                second.append(s * L + i)
        first += [s * L, s * L + n - 1]
    order = list(dict.fromkeys(first + second + list(range(len(prots) * L))))
    return np.array(sorted(order[:limit]), np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="L40,L97,B2,1BRS")
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    torch.set_num_threads(args.threads)
    sd = make_random_state_dict(WEIGHT_SEED)
    models = {}
    for prec, dt in (("32", torch.float32), ("64", torch.float64)):
        m = refshim.build_reference_module(0)
        m.load_state_dict(sd, strict=True)
        models[prec] = m.to(dt).eval()
    model = models["32"]
    from src.models.components import gather_nodes, get_atom14_coords
    from src.models.components.clash import compute_residue_clash
    from src.models.components.optimize import find_clash_mask, proximal_optimizer
    from src.datamodules.components.complex_dataset import ComplexDataset

    for tag, prots in cases().items():
        if tag not in args.only.split(","):
            continue
        out = {"n_complexes": np.int64(len(prots))}
        datas = []
        for s, prot in enumerate(prots):
            mine = protein_to_data(prot)
            ref = ComplexDataset.prot_to_data({k: (v.copy() if hasattr(v, "copy") else v) for k, v in prot.items()},
                                              cache_processed_data=False)
            for k in TENSOR_KEYS:
                assert torch.equal(ref[k], mine[k]), (tag, s, k)
                out[f"ref{s}.{k}"] = ref[k].numpy()
            for k in PROT_KEYS:
                out[f"prot{s}.{k}"] = np.asarray(prot[k])
            datas.append(mine)
        b = as_single(datas[0]) if len(datas) == 1 else collate(datas)
        rb = ref_batch(b)
        B, L = b.residue_type.shape
        out.update(pack_batch(b))
        rows = interesting_rows(prots, L, HE_ROWS)
        out["hE0_rows"] = rows
        with torch.no_grad():
            init = seeded_init(model, rb, INIT_SEED)
            out["init_chi"] = init
            enc = model.encoder
            _, E_idx, _ = enc._dist(rb.X[:, :, 1, :], rb.residue_mask)
            out["E_idx"] = E_idx
            for tval, tname in ((1.0, "t1"), (0.5, "t05"), (1.0 / 30, "t30")):
                t = torch.tensor([tval]).repeat_interleave(B * L)
                sincos = torch.stack((init.sin(), init.cos()), -1) * rb.SC_D_mask[..., None]
                h_V0, h_E0, E2, _ = enc(rb.X, rb.residue_type, rb.BB_D_sincos, sincos, rb.chain_indices, rb.residue_mask,
                                        rb.residue_index, t.clone())
                assert torch.equal(E2, E_idx)
                score, h_V = model.network(rb, init, t.clone())
                out[f"score_{tname}"] = score
                out[f"hV_{tname}"] = h_V
                if tname == "t1":
                    out["hE0"] = h_E0.reshape(B * L, *h_E0.shape[2:])[rows]
                    if tag == "L40":
                        out["hV0_t1"] = h_V0
                        ma = gather_nodes(rb.residue_mask.unsqueeze(-1), E_idx).squeeze(-1) * rb.residue_mask.unsqueeze(-1)
                        hv, he = h_V0, h_E0
                        for li, layer in enumerate(model.mpnn.mpnn_layers):
                            hv, he = layer(hv, he, E_idx, rb.X, rb.residue_mask, ma)
                            out[f"hV_l{li}_t1"] = hv
                            if li < 2:
                                out[f"hE_l{li}_t1"] = he.reshape(B * L, *he.shape[2:])[rows[:8]]
            out["atom14_init"] = get_atom14_coords(rb.X, rb.residue_type, rb.BB_D, init)
            out["clash_init"] = compute_residue_clash(rb, init, 12., 0.5)
        x = init.clone().requires_grad_(True)
        compute_residue_clash(rb, x, 12., 0.5).mean().backward()
        out["clash_grad_init"] = x.grad
        x64 = init.double().requires_grad_(True)
        compute_residue_clash(ref_batch(b, True), x64, 12., 0.5).mean().backward()
        out["clash_grad_init_fp64"] = x64.grad
        accidental = int(((x.grad == 0) != (x64.grad == 0)).sum())

        # 30 ODE steps in both precisions
        res = {}
        for prec, dt in (("32", torch.float32), ("64", torch.float64)):
            m = models[prec]
            m.schedule = torch.linspace(1, 0, N_STEPS + 1, dtype=dt)
            m.add_sc_noise = lambda bb, t, x0=init.to(dt): (x0.clone(), None)
            try:
                with torch.no_grad():
                    res[prec] = m.sampling(ref_batch(b, dt == torch.float64))
            finally:
                del m.add_sc_noise                      # the class's own method again (seeded_init draws with it)
            out[f"chi_ode_{N_STEPS}_fp{prec}"] = res[prec]
        cond = float(wrapped(res["32"], res["64"])[b.SC_D_mask.bool()].max())
        out["cond"] = np.float64(cond)

        # five proximal steps per complex (the reference's optimiser takes one protein at a time), both precisions
        moved_outside = 0
        for s, one in enumerate(split(b) if B > 1 else [b]):
            chi0 = init[s:s + 1]
            for prec, dbl in (("32", False), ("64", True)):
                r1 = ref_batch(one, dbl)
                x0 = chi0.double() if dbl else chi0.clone()
                mask = find_clash_mask(r1, x0, 12., 0.5)
                chis, losses = proximal_optimizer(r1, x0.clone(), 12., 0.5, 1., PROX_STEPS)
                out[f"prox{prec}_chi.{s}"] = torch.stack([c.detach() for c in chis])
                out[f"prox{prec}_losses.{s}"] = np.array(losses, np.float64)
                out[f"prox{prec}_mask.{s}"] = mask[..., 0]
                if not dbl:
                    moved_outside += int(((chis[-1].detach() != chi0) & (one.SC_D_mask == 0)).sum())
        g = out["clash_grad_init"]
        print(f"{tag}: B {B} L {L}  cond {cond:.2e} rad  entries outside SC_D_mask with a gradient "
              f"{int(((g != 0) & (b.SC_D_mask == 0)).sum())}, moved by the proximal run {moved_outside}, "
              f"gradient entries zero in one precision only {accidental}", flush=True)
        path = os.path.join(GOLD, f"g13_incomplete_{tag}.npz")
        np.savez_compressed(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in out.items()})
        size = os.path.getsize(path)
        print(f"  wrote {os.path.basename(path)}  {size / 1e6:.2f} MB", flush=True)
        assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
