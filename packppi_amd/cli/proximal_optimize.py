"""``proximal_optimize`` command line (src/proximal_optimize.py:26-78): clash-relax the side chains of a PDB.

Flags as in the reference (:69-78) plus --device (the reference script is CPU only; this path is HIP only).
--repack SPEC|interface (as in eval_diffusion): only the named residues may move, every other residue keeps
the input's angles (the pinned optimiser: the clash threshold is still the mean over all residues).
--obstacles hetero|hetero+water (default none: every output byte as before): the file's HETATM records and
non-standard residues become fixed obstacle atoms of the clash loss; structure.pdb keeps their lines and obstacles.csv lists every
residue's clash against them before and after.
--sasa (without it every output byte as before) writes sasa.csv for the optimised structure, as eval_diffusion
does; --repack also takes interface:sasa (the delta-SASA interface of the input, made on the device) and pocket (residues whose
surface the obstacle atoms bury; needs --obstacles other than none).
--hnet (without it every output byte as before): the hydrogen-bond network of the optimised structure is
optimised on the device -- structure.pdb takes the flips, structure_H.pdb the optimised hydrogens, hnet.csv lists the movers.
--refine_allatom (without it every output byte as before): behind the proximal stage the side chains are
refined in chi space against the explicit-hydrogen overlaps (kept rows stay) -- structure.pdb takes the refined angles, refine.csv
lists the moved residues, the --clashscore summary gains the score before and after.
--anchors auto|geometry|SPEC (without it every output byte as before): in front of the optimiser the side chains
that coordinate a metal or are covalently linked to a ligand are closed onto it from the input's angles; the optimiser then keeps
them.  Writes anchors.csv and, with --obstacles, LINK records at the head of structure.pdb, as eval_diffusion does.
--clashscore / --hydrogens (without them every output byte as before): clashes.csv (every serious all-atom
overlap of the optimised structure with placed hydrogens, kept | gained | lost against the input, and the clashscore of both) and
structure_H.pdb, as eval_diffusion writes them.  Not MolProbity's score.
"""
import argparse
from pathlib import Path

from ..analysis import ProteinAnalysis
from ..functional import get_atom14_coords, proximal_optimizer
from ..pdb_io import OBSTACLE_MODES, contains_sidechains, from_pdb_file, insert_obstacle_lines, obstacles_for, to_pdb


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--input", type=str, help="The input pdb file path.", required=True)
    p.add_argument("--outdir", type=str, help="Directory to store outputs.", required=True)
    p.add_argument("--molprobity_clash_loc", type=str, help="Path to /build/bin/molprobity.clashscore.", required=True)
    p.add_argument("--violation_tolerance_factor", type=float, help="The violation tolerance factor.", default=12)
    p.add_argument("--clash_overlap_tolerance", type=float, help="Acceptable deviation between atoms.", default=0.5)
    p.add_argument("--lamda", type=float, help="The influence of the proximal term on the gradient.", default=1)
    p.add_argument("--num_steps", type=int, help="Number of optimize steps.", default=50)
    p.add_argument("--device", type=str, default="cuda")
    p.add_argument("--repack", type=str, default=None, metavar="SPEC|interface", help="Optimise only these residues, e.g. "
                   "'A:45-60,B:12,C' (chain and PDB residue number) or 'interface'; the others keep the input's angles.")
    p.add_argument("--obstacles", choices=OBSTACLE_MODES, default="none", help="Fixed atoms the clash stages keep the side chains off (DESIGN.md section 19): none (default), hetero = every HETATM record and "
                   "every non-standard residue (ligands, cofactors, nucleic acids; no hydrogens, waters or metals), hetero+water = the "
                   "waters too. The diffusion network does not see them: the clash stages of this tool repair"
                   " what it puts into the pocket. Written structures keep the records.")
    p.add_argument("--sasa", action="store_true", help="Write sasa.csv for the optimised structure (DESIGN.md section 20): per "
                   "residue the solvent-accessible area at four nested levels, the buried interface area and the exposure. --repack "
                   "also takes interface:sasa and pocket (needs --obstacles).")
    from .eval_diffusion import add_allatom_arguments, add_anchor_arguments
    add_allatom_arguments(p)
    add_anchor_arguments(p)
    return p


def parse_args(argv=None):
    from ..selection import device_selector
    p = build_parser()
    args = p.parse_args(argv)
    try:
        device_selector(args.repack, args.obstacles)
    except ValueError as e:
        p.error(str(e))
    return args


def main(argv=None):
    args = parse_args(argv)

    assert contains_sidechains(args.input), "----- No side chain atoms found in the input PDB -----"
    print("----- Starting optimize! -----")
    analysis = ProteinAnalysis(args.molprobity_clash_loc, args.outdir, args.device)
    print(f"----- The input structure clashscore is {analysis.get_clashscore(args.input)} -----")
    protein = from_pdb_file(Path(args.input), mse_to_met=True)
    obstacles = obstacles_for(args.input, args.obstacles)
    batch = analysis.get_prot(args.input)
    if obstacles is not None:
        from ..featurize import _add_obstacles
        _add_obstacles(batch, obstacles)
    batch = batch.to(args.device)
    fixed = None
    if args.repack is not None:
        import torch
        from ..selection import device_selector, interface_selection, parse_selection, sasa_selection
        kind = device_selector(args.repack, args.obstacles)
        if kind is not None:
            sel = sasa_selection(batch, kind)
        else:
            sel = interface_selection(protein, args.input) if args.repack == "interface" else parse_selection(args.repack, protein)
        print(f"----- Optimising {int(sel.sum())} of {len(sel)} residues; the others keep the input's angles -----")
        fixed = torch.from_numpy(~sel).unsqueeze(0)
    start, links = batch.SC_D, ""
    if hasattr(args, "anchors"):
        # closed from the input's angles, then held: the optimiser's accept rule compares the closed structure with the optimised one
        from ..functional import _ctx_for
        from ..pdb_io import anchor_sites
        from .eval_diffusion import anchors_from_args, write_anchors
        a = anchors_from_args(args, protein=protein)
        a = anchor_sites(args.input, protein, "link", log=print) if isinstance(a, str) else a
        ctx = _ctx_for(batch)
        res = ctx.anchors(batch.SC_D, a.shifted(0, 0), fixed=fixed, names=[f"{c}:{int(n)}" for c, n in zip(protein["chain_id"], protein["residue_index"])])
        links = write_anchors(dict(res, anchors=a, chi_before=batch.SC_D), ctx, protein, args.outdir, args.input, obstacles is not None)
        start = res.chi
        held = res.pinned().reshape(1, -1)
        fixed = held if fixed is None else held | (fixed.to(held.device) != 0)
    chis, losses = proximal_optimizer(batch, start, args.violation_tolerance_factor,
                                      args.clash_overlap_tolerance, args.lamda, args.num_steps, fixed_mask=fixed)
    SC_D = chis[-1] if losses[-1] < losses[0] else start
    xyz = get_atom14_coords(batch.X, batch.residue_type, batch.BB_D, SC_D)
    protein["atom_positions"] = xyz.cpu().squeeze(0).numpy()
    with open(analysis.tmp_pdb, "w") as fh:
        fh.writelines(links + insert_obstacle_lines(to_pdb(protein), obstacles["lines"] if obstacles else []))
    if obstacles is not None:
        import os
        from ..functional import _ctx_for
        kw = dict(vtf=args.violation_tolerance_factor, tol=args.clash_overlap_tolerance)
        ctx, shares = _ctx_for(batch), []
        for chi in (batch.SC_D, SC_D):
            with_set = ctx.clash(chi, **kw)
            ctx.set_obstacles(None)
            shares.append((with_set - ctx.clash(chi, **kw))[0].cpu().tolist())
            ctx.set_obstacles(batch.obstacle_xyzr, ctx._obstacle_ranges(batch), polar=batch.get("obstacle_polar"))
        with open(os.path.join(args.outdir, "obstacles.csv"), "w") as fh:
            fh.write("residue,chain,clash_obstacles_before,clash_obstacles_after\n")
            for num, cid, b, a in zip(protein["residue_index"], protein["chain_id"], *shares):
                fh.write(f"{int(num)},{cid},{b!r},{a!r}\n")
    if args.sasa:
        from .eval_diffusion import write_sasa
        write_sasa(batch, protein, args.outdir, SC_D)
    unrefined = None
    if getattr(args, "refine_allatom", False):
        # structure.pdb takes the refined angles; kept rows (--repack) stay
        import os
        from ..analysis import write_refine
        from ..functional import _ctx_for
        unrefined = SC_D
        res = _ctx_for(batch).refine_allatom(SC_D, fixed=fixed)
        write_refine(os.path.join(args.outdir, "refine.csv"), protein, res)
        SC_D = res.chi[:, :SC_D.shape[1]].to(SC_D.device)
        refined = dict(protein, atom_positions=get_atom14_coords(batch.X, batch.residue_type, batch.BB_D, SC_D).cpu().squeeze(0).numpy())
        with open(analysis.tmp_pdb, "w") as fh:
            fh.writelines(links + insert_obstacle_lines(to_pdb(refined), obstacles["lines"] if obstacles else []))
    hnet = None
    if getattr(args, "hnet", False):
        # structure.pdb takes the flips: written again at the angles of the optimised network
        from .eval_diffusion import optimise_hnet
        hnet = optimise_hnet(batch, protein, args.outdir, SC_D)
        SC_D = hnet.chi[:, :SC_D.shape[1]].to(SC_D.device)
        flipped = dict(protein, atom_positions=get_atom14_coords(batch.X, batch.residue_type, batch.BB_D, SC_D).cpu().squeeze(0).numpy())
        with open(analysis.tmp_pdb, "w") as fh:
            fh.writelines(links + insert_obstacle_lines(to_pdb(flipped), obstacles["lines"] if obstacles else []))
    if getattr(args, "clashscore", False) or getattr(args, "hydrogens", False):
        from .eval_diffusion import write_allatom
        write_allatom(batch, protein, args.outdir, SC_D, getattr(args, "clashscore", False), getattr(args, "hydrogens", False),
                      native=True, obstacle_lines=obstacles["lines"] if obstacles else [], **(dict(hnet=hnet) if hnet is not None else {}),
                      **(dict(unrefined=unrefined) if unrefined is not None else {}))
    print(f"----- The optimized structure clashscore is {analysis.get_clashscore(analysis.tmp_pdb)} -----")
    print("----- Finishing optimize! -----")


if __name__ == "__main__":
    main()
