"""``mutate`` command line: PDB + mutation sets in -> one repacked mutant structure per set (``TDiffusionModule.mutate``,
DESIGN.md section 17).

    python -m packppi_amd.cli.mutate --input x.pdb (--mutstr RA47A,EA48A | --mutlist FILE) --ckpt_path model.ckpt --seed 7
        [--n_decoys 8] [--select clash|medoid] [--use_proximal] [--radius 10] [--shell ca|atom] [--fixed_mode hold|renoise]
        [--recombine [--recombine_sweeps 64]] [--guide 0.02 [--guide_schedule late|constant] [--guide_from 0.3] [--guide_cap 0.1]]
        [--corrector 0.16 [--corrector_from 1.0]]
        --outdir out [--ap_ckpt ap.ckpt --pre_ckpt_path pre.ckpt]

Every set is put into the complex, the residues within --radius of a mutated residue (the shell, chosen on the device) are
repacked around the new side chains, every other residue keeps the input's angles bit for bit.  All sets go through one packed
pass.  Writes ``mutant_<tag>.pdb`` per set (the mutant's residue names and atoms) and ``mutants.csv``.  --mutlist FILE: one set
per line, comma-separated as --mutstr, ``#`` lines skipped (the format of eval_affinity --mutlist).  --recombine: the decoys of
every set are recombined per residue by clash descent from the selected one; ``mutant_<tag>.pdb`` is then the
recombined structure and ``mutants.csv`` gains the columns ``clash_recombined`` and ``rows_recombined``.
--obstacles hetero|hetero+water (default none: every output byte as before): the file's HETATM records and
non-standard residues become fixed obstacle atoms of every clash stage (--use_proximal, the clash ranking, --recombine); the
network does not see them.  Every ``mutant_<tag>.pdb`` keeps their lines and ``obstacles.csv`` lists, per set and residue, the
clash against them at the wild type's angles (new side chains at chi = 0) and at the result's.
--sasa (without it every output byte as before): next to every ``mutant_<tag>.pdb`` a ``sasa_<tag>.csv`` of
that structure (per residue the solvent-accessible area at four nested levels, the buried interface area and the exposure; the file
``eval_diffusion --sasa`` writes as sasa.csv), and ``mutants.csv`` gains the column ``bsa``, the interface area the selected decoy
buries.
--hnet (without it every output byte as before): every mutant's hydrogen-bond network is optimised on the
device -- ``mutant_<tag>.pdb`` takes the flips, ``mutant_<tag>_H.pdb`` the optimised hydrogens, ``hnet_<tag>.csv`` lists the movers and
mutants.csv gains hnet_bonds and hnet_flips (with --clashscore also clashscore_hnet) of the selected decoy.
--refine_allatom (without it every output byte as before): the shell rows of every decoy are refined in chi
space against the explicit-hydrogen overlaps behind the pinned stage; mutants.csv gains refine_moved, refine_F_before and
refine_F_after of the selected decoy, ``refine_<tag>.csv`` lists the residues its refinement moved, and the --clashscore summary
gains the score before and after.
--clashscore / --hydrogens (without them every output byte as before): next to every ``mutant_<tag>.pdb`` a
``clashes_<tag>.csv`` (every serious all-atom overlap with placed hydrogens; mutants.csv gains the columns clashscore and
clashes_interface of the selected decoy) and a ``mutant_<tag>_H.pdb`` (the mutant plus the placed hydrogens).  Not MolProbity's score.
--polar (without it every output byte as before): next to every ``mutant_<tag>.pdb`` a ``polar_<tag>.csv`` and a
``hbonds_<tag>.csv`` of that structure (the files ``eval_diffusion --polar`` writes as polar.csv and hbonds.csv, without the
comparison against the input: the mutant has other side chains), and ``mutants.csv`` gains the columns ``hbonds``,
``hbonds_interface``, ``salt_interface`` and, with --sasa, ``buns_interface`` of the selected decoy.
--guide SCALE ... (without it every output byte as before): the shell is sampled with clash guidance, as
``eval_diffusion --guide``; ``guide.csv`` has one block of lines per decoy of every set.
--corrector SNR [--corrector_from T] (without it every output byte as before): the shell is sampled with a
Langevin corrector behind the reverse steps, as ``eval_diffusion --corrector``; ``corrector.csv`` has one block per decoy of every set.
"""
import argparse
import os

import numpy as np

from ..featurize import parse_mutstr
from ..pdb_io import OBSTACLE_MODES, from_pdb_file, insert_obstacle_lines, obstacles_for, to_pdb
from .eval_diffusion import (add_corrector_arguments, add_guide_arguments, corrector_from_args, guide_from_args, load_model,
                             write_corrector_csv, write_guide_csv)

AP_NOTE = ("The ddG values come from the unchanged AffinityPrediction.predict_many on featurize.mutant_data. The AP model was "
           "trained with zeroed mutant angles, so it does not see the packed mutant.")


def read_sets(args):
    if args.mutlist:
        with open(args.mutlist) as fh:
            return [ln.strip() for ln in fh if ln.strip() and not ln.lstrip().startswith("#")]
    return [args.mutstr]


def predict_ddg(protein, sets, args):
    """(ddg, ddg_inv) lists of PackPPI-AP for the sets, from the wild type and the zero-angle mutant of ``mutant_data``."""
    from ..affinity import AffinityPrediction
    from ..featurize import mutant_data
    print(f"----- Loading {args.ap_ckpt} checkpoint! -----")
    ap = AffinityPrediction.load_from_checkpoint(args.ap_ckpt, pre_checkpoint_path=args.pre_ckpt_path, map_location=args.device).eval()
    ddg, inv = ap.predict_many([mutant_data(protein, parse_mutstr(s)) for s in sets])
    return ddg.cpu().tolist(), inv.cpu().tolist()


def evaluate_model(model, args):
    print("----- Starting evaluation! -----")
    os.makedirs(args.outdir, exist_ok=True)
    protein = from_pdb_file(args.input, mse_to_met=True)
    protein["pdb_path"] = args.input
    obstacles = obstacles_for(args.input, args.obstacles)
    if obstacles is not None:
        protein["obstacles"] = obstacles
    ob_rows = ["tag,residue,chain,clash_obstacles_before,clash_obstacles_after"]
    sets = read_sets(args)
    guide = guide_from_args(args)
    model.keep_guide_trace = guide is not None
    corrector = corrector_from_args(args)
    model.keep_corrector_trace = corrector is not None
    polar = getattr(args, "polar", False)
    pcols = ("hbonds", "hbonds_interface", "salt_interface") + (("buns_interface",) if args.sasa else ()) if polar else ()
    allatom, with_h, hnet_on = getattr(args, "clashscore", False), getattr(args, "hydrogens", False), getattr(args, "hnet", False)
    hcols = (("hnet_bonds", "hnet_flips") + (("clashscore_hnet",) if allatom else ())) if hnet_on else ()
    refine_on = getattr(args, "refine_allatom", False)
    results = model.mutate([(protein, s) for s in sets], seed=args.seed, radius=args.radius, shell=args.shell,
                           n_decoys=args.n_decoys, use_proximal=args.use_proximal, select=args.select, fixed_mode=args.fixed_mode,
                           **(dict(recombine=True, recombine_sweeps=args.recombine_sweeps) if args.recombine else {}),
                           **(dict(sasa=True) if args.sasa else {}), **(dict(polar=True) if polar else {}), **(dict(clashscore=True) if allatom else {}),
                           **(dict(hbond_optimize=True) if hnet_on else {}), **(dict(refine_allatom=True) if refine_on else {}),
                           **(dict(guide=guide) if guide is not None else {}),
                           **(dict(corrector=corrector) if corrector is not None else {}))
    if guide is not None:
        write_guide_csv(model, args.outdir)
    if corrector is not None:
        write_corrector_csv(model, args.outdir)
    ddg = predict_ddg(protein, sets, args) if args.ap_ckpt else None
    rows = ["tag,shell_rows,selected_decoy,clash,dev" + (",clash_recombined,rows_recombined" if args.recombine else "")
            + (",ddg,ddg_inv" if ddg else "") + (",bsa" if args.sasa else "") + "".join("," + k for k in pcols)
            + (",clashscore,clashes_interface" if allatom else "") + "".join("," + k for k in hcols)
            + (",refine_moved,refine_F_before,refine_F_after" if refine_on else "")]
    for i, (s, r) in enumerate(zip(sets, results)):
        tag = (r["tag"] or s).replace(",", "_")
        b = r["batch"]
        mutant = dict(protein, atom_positions=r["X"][0].cpu().numpy(), atom_mask=b["atom_mask"][0].cpu().numpy(),
                      aaindex=np.where(b["residue_mask"][0].cpu().numpy() > 0, b["residue_type"][0].cpu().numpy(),
                                       np.asarray(protein["aaindex"])))
        unrefined = None
        if refine_on:                            # what the selected decoy's refinement did, row by row
            from ..analysis import refine_csv
            unrefined = r["refine_chi0"]
            with open(os.path.join(args.outdir, f"refine_{tag}.csv"), "w") as fh:
                fh.write(refine_csv(mutant["aaindex"], r["refine_steps"][:, 0].cpu().numpy(), [float(np.rad2deg(d)) for d in r["refine_deltas"]],
                                    r["refine_e"][0].cpu().numpy(), protein["chain_id"], protein["residue_index"]))
        hnet = None
        if hnet_on:                              # the mutant's file takes the flips of its optimised network
            from .eval_diffusion import optimise_hnet
            hnet = optimise_hnet(b, mutant, args.outdir, r["SC_D"], name=f"hnet_{tag}.csv")
            r["SC_D"] = hnet.chi
            mutant = dict(mutant, atom_positions=hnet.xyz[0].cpu().numpy())
        with open(os.path.join(args.outdir, f"mutant_{tag}.pdb"), "w") as fh:
            fh.write(insert_obstacle_lines(to_pdb(mutant), obstacles["lines"] if obstacles else []))
        if obstacles is not None:
            from .eval_diffusion import obstacle_share
            before, after = obstacle_share(model, b, b["SC_D"]), obstacle_share(model, b, r["SC_D"])
            ob_rows += [f"{tag},{int(num)},{cid},{x!r},{y!r}" for num, cid, x, y in
                        zip(protein["residue_index"], protein["chain_id"], before, after)]
        best = int(r["best"])
        line = f"{tag},{int(r['shell'].sum())},{best},{float(r['clash'][best])!r},{float(r['dev'][best])!r}"
        if args.recombine:
            line += f",{float(r['clash_recombined'])!r},{int(r['rows_recombined'])}"
        if ddg:
            line += f",{ddg[0][i]!r},{ddg[1][i]!r}"
        if args.sasa:
            from .eval_diffusion import write_sasa
            line += f",{float(r['bsa'][best])!r}"
            write_sasa(b, mutant, args.outdir, r["SC_D"], name=f"sasa_{tag}.csv")
        if polar:
            from .eval_diffusion import write_polar
            line += "".join(f",{int(r[k][best])}" for k in pcols)
            write_polar(b, mutant, args.outdir, r["SC_D"], sasa=args.sasa,
                        names=(f"polar_{tag}.csv", f"hbonds_{tag}.csv"))
        if allatom or with_h:
            from .eval_diffusion import write_allatom
            if allatom:
                line += f",{float(r['clashscore'][best])!r},{int(r['clashes_interface'][best])}"
            write_allatom(b, mutant, args.outdir, r["SC_D"], allatom, with_h, obstacle_lines=obstacles["lines"] if obstacles else [],
                          names=(f"clashes_{tag}.csv", f"mutant_{tag}_H.pdb"), **(dict(hnet=hnet) if hnet is not None else {}),
                          **(dict(unrefined=unrefined) if unrefined is not None else {}))
        for k in hcols:
            line += f",{float(r[k][best])!r}" if k == "clashscore_hnet" else f",{int(r[k][best])}"
        if refine_on:
            line += f",{int(r['refine_moved'][best])},{int(r['refine_F'][best, 0])},{int(r['refine_F'][best, 1])}"
        rows.append(line)
        print(f"----- {tag}: {int(r['shell'].sum())} residues repacked, decoy {best} of {args.n_decoys} selected"
              + (f", {int(r['rows_recombined'])} residues recombined from other decoys" if args.recombine else "") + " -----")
    with open(os.path.join(args.outdir, "mutants.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")
    if obstacles is not None:
        with open(os.path.join(args.outdir, "obstacles.csv"), "w") as fh:
            fh.write("\n".join(ob_rows) + "\n")
    if model.saturated():
        print("----- WARNING: sticky flag %d (f16 saturation or non-finite input) in the score network -----" % model.saturated())
    print("----- Finishing evaluation! -----")


def build_parser():
    p = argparse.ArgumentParser(description="Model mutants: repack the shell around each mutation set. " + AP_NOTE)
    p.add_argument("--input", type=str, help="The input pdb file path.", required=True)
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--mutstr", type=str, help='One mutation set: wild-type residue, chain ID, position and mutant residue, several '
                   'separated by commas (e.g. "RA47A,EA48A").')
    g.add_argument("--mutlist", type=str, help="File with one mutation set per line (as eval_affinity --mutlist); all sets run in "
                   "one packed pass.")
    p.add_argument("--outdir", type=str, help="Directory to store outputs.", required=True)
    p.add_argument("--device", type=str, help="cuda (the MI355X HIP device)", default="cuda")
    p.add_argument("--ckpt_path", type=str, default=None, help="Lightning checkpoint of the score network (else $PACKPPI_CKPT, else "
                   "the config tree's ckpt_path).")
    p.add_argument("--config_dir", type=str, default=None, help="The reference's configs/ directory (else $PACKPPI_CONFIG_DIR).")
    p.add_argument("--steps", type=int, default=None, help="Diffusion steps (reference schedule: 30).")
    p.add_argument("--random_weights", type=int, default=None, help="Seeded stand-in weights instead of a checkpoint.")
    p.add_argument("--seed", type=int, required=True, help="Seed of the sampling noise, drawn by the counter-based generator on the "
                   "device; set i of the call has the noise key i.")
    p.add_argument("--n_decoys", type=int, default=1, metavar="D", help="Decoys per set, drawn in one packed pass; the selected one "
                   "is written.")
    p.add_argument("--select", choices=("clash", "medoid"), default="clash", help="Keep the decoy with the lowest mean clash (clash) "
                   "or the one closest to the circular consensus (medoid).")
    p.add_argument("--use_proximal", action="store_true", help="Run the pinned proximal clash optimisation on the shell.")
    p.add_argument("--recombine", action="store_true", help="Recombine the decoys per residue by clash descent from the selected "
                   "one; the written mutant is the recombined structure.")
    p.add_argument("--recombine_sweeps", type=int, default=64, metavar="K", help="With --recombine: the largest number of sweeps.")
    p.add_argument("--radius", type=float, default=10.0, help="Shell radius in Angstrom.")
    p.add_argument("--shell", choices=("ca", "atom"), default="ca", help="Shell rule: CA within the radius of a mutated CA (ca, the "
                   "local subgraph of PackPPI-AP) or any atom within it of an atom of a mutated residue (atom).")
    p.add_argument("--fixed_mode", choices=("hold", "renoise"), default="renoise", help="What the kept residues look like to the "
                   "network during sampling: re-noised to each step's level (renoise) or clean throughout (hold).")
    p.add_argument("--ap_ckpt", type=str, default=None, help="AffinityPrediction checkpoint: adds ddg and ddg_inv to mutants.csv. "
                   + AP_NOTE)
    p.add_argument("--pre_ckpt_path", type=str, default=None, help="With --ap_ckpt: the pretrained PackPPI checkpoint (default: the "
                   "one named in the AP checkpoint's hyper_parameters).")
    p.add_argument("--obstacles", choices=OBSTACLE_MODES, default="none", help="Fixed atoms the clash stages keep the side chains off (DESIGN.md section 19): none (default), hetero = every HETATM record and "
                   "every non-standard residue (ligands, cofactors, nucleic acids; no hydrogens, waters or metals), hetero+water = the "
                   "waters too. The diffusion network does not see them: sampling is unchanged, the clash stages (--use_proximal, "
                   "decoy ranking, --recombine) repair what it puts into the pocket. Written structures keep the records.")
    p.add_argument("--sasa", action="store_true", help="Write sasa_<tag>.csv next to every mutant (DESIGN.md section 20): per residue "
                   "the solvent-accessible area at four nested levels, the buried interface area and the exposure; mutants.csv gains "
                   "the column bsa.")
    p.add_argument("--polar", action="store_true", default=argparse.SUPPRESS, help="Write polar_<tag>.csv and hbonds_<tag>.csv next "
                   "to every mutant (DESIGN.md section 27): hydrogen bonds, salt bridges and polar atoms without a partner; "
                   "mutants.csv gains the columns hbonds, hbonds_interface, salt_interface and, with --sasa, buns_interface.")
    add_guide_arguments(p)
    add_corrector_arguments(p)
    from .eval_diffusion import add_allatom_arguments
    add_allatom_arguments(p)
    return p


def main(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    if args.n_decoys < 1:
        p.error("--n_decoys must be at least 1")
    if args.recombine_sweeps < 0:
        p.error("--recombine_sweeps must not be negative")
    if args.pre_ckpt_path and not args.ap_ckpt:
        p.error("--pre_ckpt_path belongs to --ap_ckpt")
    guide_from_args(args, p)
    corrector_from_args(args, p)
    evaluate_model(load_model(args), args)


if __name__ == "__main__":
    main()
