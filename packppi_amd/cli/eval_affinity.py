"""``eval_affinity`` command line: PDB + mutation string in -> predicted binding ddG (PackPPI-AP).

Same flags as the reference's src/eval_affinity.py:95-100 (--input, --mutstr, --device) and the same result line.  The
reference takes both checkpoint paths from configs/eval_affinity.yaml through Hydra; here --ckpt_path / --pre_ckpt_path
name them (--config_dir: a configs/ tree whose encoder / model YAML files are checked against the compiled dimensions, as
in cli.eval_diffusion), or --random_weights SEED uses seeded stand-ins for both.  --mode overrides the checkpoint's
hyper_parameters.mode.  --mutlist FILE evaluates one mutation set per line (comma-separated, as --mutstr) in one packed
batch and prints one result line per set, in file order.
"""
import argparse
import os

from ..affinity import AffinityPrediction
from ..featurize import mutant_data, parse_mutstr
from ..batch import as_single
from ..pdb_io import from_pdb_file

RESULT = "----- The predicted binding affinity change (wildtype-mutant) is {:.4f} kcal/mol -----"


def load_model(args):
    cfg_kw = {}
    if args.config_dir:
        from ..config import load_hot_path_configs
        cfgs = load_hot_path_configs(args.config_dir)
        cfg_kw = dict(encoder_cfg=cfgs.encoder_cfg, model_cfg=cfgs.model_cfg)
    if args.random_weights is not None:
        from ..weights import make_random_affinity_state_dict, make_random_state_dict
        mode = args.mode or "network"
        print(f"----- Using seeded random weights (seed {args.random_weights}); no checkpoint given! -----")
        return AffinityPrediction(make_random_affinity_state_dict(args.random_weights, mode),
                                  make_random_state_dict(args.random_weights), mode=mode, device=args.device, **cfg_kw)
    assert args.ckpt_path is not None and os.path.exists(args.ckpt_path), "Invalid checkpoint path!"
    print(f"----- Loading {args.ckpt_path} checkpoint! -----")
    return AffinityPrediction.load_from_checkpoint(args.ckpt_path, pre_checkpoint_path=args.pre_ckpt_path,
                                                   map_location=args.device, mode=args.mode, **cfg_kw).eval()


def evaluate_model(model, args):
    print("----- Starting evaluation! -----")
    protein = from_pdb_file(args.input, mse_to_met=True)
    protein["pdb_path"] = args.input
    if args.mutlist:
        with open(args.mutlist) as fh:
            sets = [ln.strip() for ln in fh if ln.strip() and not ln.lstrip().startswith("#")]
        datas = [mutant_data(protein, parse_mutstr(s)) for s in sets]
        ddg, _ = model.predict_many(datas)
        for s, v in zip(sets, ddg.cpu().tolist()):
            print(f"{s}\t" + RESULT.format(v))
    else:
        batch = as_single(mutant_data(protein, parse_mutstr(args.mutstr))).to(args.device)
        _, pred = model.forward(batch)
        print(RESULT.format(pred.cpu().item()))
    if model.saturated():
        print("----- WARNING: sticky flag %d (f16 saturation or non-finite input) in the networks -----" % model.saturated())
    print("----- Finishing evaluation! -----")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--input", type=str, help="The input pdb file path.", required=True)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--mutstr", type=str, help='Wild-type residue, chain ID, position and mutant residue (e.g. "RA47A"); '
                   'several mutations separated by commas (e.g. "RA47A,EA48A").')
    g.add_argument("--mutlist", type=str, help="File with one mutation string per line, evaluated as one packed batch.")
    p.add_argument("--device", type=str, help="cuda (the MI355X HIP device)", default="cuda")
    p.add_argument("--ckpt_path", type=str, default=None, help="AffinityPrediction Lightning checkpoint.")
    p.add_argument("--pre_ckpt_path", type=str, default=None,
                   help="Pretrained PackPPI checkpoint (default: the one named in the checkpoint's hyper_parameters).")
    p.add_argument("--config_dir", type=str, default=None, help="The reference's configs/ directory: encoder / model YAML "
                   "files are checked against the compiled dimensions.")
    p.add_argument("--mode", type=str, default=None, choices=("network", "linear", "esm"),
                   help="Override the checkpoint's mode (esm is not supported).")
    p.add_argument("--random_weights", type=int, default=None, help="Seeded stand-in weights instead of checkpoints.")
    args = p.parse_args(argv)
    evaluate_model(load_model(args), args)


if __name__ == "__main__":
    main()
