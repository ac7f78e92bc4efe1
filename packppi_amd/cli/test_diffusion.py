"""``test_diffusion`` command line: PDB files in -> the denoising score-matching loss ``trainer.test`` reports as ``test/loss``.

The reference runs ``trainer.test`` over its test split (src/eval.py, TorsionalDiffusion.py:214-229): ``test_step`` per batch,
a mean over batches.  Here the inputs are packed into one batch (every complex computed as if alone), each complex draws its
own t, and the loss is repeated ``--repeats`` times; ``test/loss`` is the mean over complexes and repeats, and one line per
complex follows.  --ckpt_path / --config_dir as in cli.eval_diffusion; --random_weights SEED uses seeded stand-in weights.
--score_norm names an ``.npy`` with the two ``score_norm_`` tables [2, 5001] of a reference run; without it they are estimated
as the reference estimates them (10000 draws per grid point; seeded by --seed).
"""
import argparse

import numpy as np
import torch

from ..batch import pack
from ..featurize import protein_to_data
from ..pdb_io import from_pdb_file
from .eval_diffusion import load_model


def packed_inputs(paths, device):
    return pack([protein_to_data(from_pdb_file(p, mse_to_met=True)) for p in paths]).to(device)


def test_loss(model, batch, seed=None, repeats=1):
    """-> [repeats, n_complexes] fp64 per-complex losses.  ``seed``: seeds NumPy (the score_norm estimate, if the model has no
    tables yet) and torch (t on the CPU, the noise on the device)."""
    if seed is not None:
        np.random.seed(seed)
        torch.manual_seed(seed)
    return torch.stack([model.forward(batch, per_complex=True) for _ in range(repeats)])


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--input", type=str, nargs="+", help="The input pdb file paths (with side chains).", required=True)
    p.add_argument("--device", type=str, help="cuda (the MI355X HIP device)", default="cuda")
    p.add_argument("--ckpt_path", type=str, default=None, help="Lightning checkpoint (else $PACKPPI_CKPT, else the config tree's ckpt_path).")
    p.add_argument("--config_dir", type=str, default=None, help="The reference's configs/ directory (else $PACKPPI_CONFIG_DIR).")
    p.add_argument("--seed", type=int, default=None, help="Seed of NumPy and torch: the score_norm estimate, t and the noise.")
    p.add_argument("--repeats", type=int, default=1, help="Loss evaluations per complex, each with a new t and noise.")
    p.add_argument("--score_norm", type=str, default=None, help=".npy with the score_norm_ tables [2, 5001] (1pi, 2pi) of a reference run.")
    p.add_argument("--random_weights", type=int, default=None, help="Seeded stand-in weights instead of a checkpoint.")
    args = p.parse_args(argv)
    if args.repeats < 1:
        p.error("--repeats must be at least 1")
    args.steps = None
    model = load_model(args)
    if args.score_norm:
        model.set_score_norm(args.score_norm)
    print("----- Starting evaluation! -----")
    losses = test_loss(model, packed_inputs(args.input, args.device), args.seed, args.repeats).cpu()
    print(f"test/loss {losses.mean().item():.6f}")
    for path, v in zip(args.input, losses.mean(0).tolist()):
        print(f"{path}\t{v:.6f}")
    if model.saturated():
        print("----- WARNING: sticky flag %d (f16 saturation or non-finite input) in the score network -----" % model.saturated())
    print("----- Finishing evaluation! -----")


if __name__ == "__main__":
    main()
