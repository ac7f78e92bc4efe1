"""``eval_diffusion`` command line: PDB in -> sampled side chains -> OUTDIR/structure.pdb + metrics.

Same required flags as the reference's src/eval_diffusion.py:86-93 (--input, --outdir, --molprobity_clash_loc,
--use_proximal, --device).  The reference composes configs/eval_diffusion.yaml with Hydra and takes its checkpoint path and
the encoder / model / sampling settings from there (eval_diffusion.py:22-41); here --config_dir (or $PACKPPI_CONFIG_DIR)
names that configs/ directory and the four hot-path YAML files are read as plain YAML (packppi_amd/config.py): sample_cfg
(mode, annealed_temp, proximal parameters) is applied, the dimensions are checked against what the kernels are compiled for.
--ckpt_path / $PACKPPI_CKPT override the tree's ckpt_path; --steps exposes the number of diffusion steps (reference: 30);
--seed N makes the run reproducible: all sampling noise then comes from the seeded device generator.
--repack SPEC|interface repacks only the named residues ("A:45-60,B:12,C": chain and PDB residue number; "interface": residues
within 10 A of another chain) and keeps every other residue at the input's angles; --fixed_mode chooses
what the sampled residues are conditioned on.  It needs --seed; with --use_proximal the proximal stage is the pinned one
(TDiffusionModule.repack): only repacked residues move, the kept ones stay at the input's angles.
--n_decoys D draws D seeded decoys in one packed pass (TDiffusionModule.sample_ensemble) and writes
OUTDIR/decoy_000.pdb ..., structure.pdb (the decoy --select picks: lowest mean clash, or the medoid), ensemble.csv (decoy, key, dev,
clash, selected) and confidence.csv (chain, residue number, residue name, resultant length of chi 1..4).  It needs --seed, combines
with --use_proximal and is refused together with --repack.
--recombine (with --n_decoys) recombines the decoys per residue by clash descent from the selected one, at most
--recombine_sweeps sweeps: recombined.pdb, recombine.csv (chain, residue number, residue name, the decoy the residue was taken from,
its local clash energy before and after) and structure.pdb = recombined.pdb; the other files are as without the flag.
--obstacles hetero|hetero+water (default none: every output byte as before): the file's HETATM records and
non-standard residues -- ligands, cofactors, nucleic acids, with hetero+water the waters -- become fixed obstacle atoms of every
clash stage (--use_proximal, the clash ranking of --n_decoys, --recombine).  The diffusion network itself does NOT see them:
sampling is unchanged, the clash stages repair what it puts into the pocket.  Every structure file written gets those records'
original lines, verbatim, between the protein's last TER and END, and obstacles.csv lists per residue its clash against the
obstacles (Context.clash with the set minus Context.clash without it) at the input's angles and at the result's.
--sasa (without it every output byte as before) writes sasa.csv for the structure written as structure.pdb:
chain, number, name, the solvent-accessible area of every residue next to itself alone, in its isolated chain, in the complex and
with the obstacle atoms, the buried interface area (chain minus complex) and the exposure (last over first); with --n_decoys
ensemble.csv gains the column bsa, the interface area every decoy buries.  The areas belong to this radius set (element van der
Waals radii, heavy atoms, probe 1.4 A, 96 points): they are not freesasa's numbers.
--repack interface:sasa selects the delta-SASA interface of the input structure -- residues with surface that is exposed in the
isolated chain and buried in the complex, the reference's interface.py rule -- on the device, without reading the file again;
--repack pocket selects the residues whose surface the obstacle atoms bury and needs --obstacles other than none.
--guide SCALE [--guide_schedule late|constant] [--guide_from T] [--guide_cap RAD] (without --guide every output
byte as before): clash-guided sampling -- between the network evaluations the angles take a gradient step of size SCALE on the clash
loss, obstacle atoms included, at most RAD radians per angle, from time T of the schedule on (late) or at every step (constant).  The
defaults (0.02, late from 0.3, 0.1 rad) are starting values, not tuned against a trained checkpoint.  Combines with --repack,
--n_decoys and --use_proximal; needs --seed with --repack and in sde mode.  Writes guide.csv (complex or decoy, nudge point, t, eta,
mean clash in front of that nudge; empty where no nudge runs) and prints the first and last traced clash.
--corrector SNR [--corrector_from T] (without --corrector every output byte as before): predictor-corrector
sampling -- behind every reverse step but the last, from time T of the schedule on (default 1: everywhere), one more network
evaluation and a Langevin step of signal-to-noise ratio SNR with a step size per complex.  0.16 is the reference's constant
(step_correct); nothing here is tuned against a trained checkpoint.  Needs --seed; combines with --repack, --n_decoys, --guide and
--use_proximal.  Writes corrector.csv (step, t, complex or decoy, s2, n2, eps, amp; empty where no corrector ran).
--refine_allatom (without it every output byte as before): the side chains are refined in chi space against
the explicit-hydrogen overlaps, behind the proximal stage and the disulfide closure and in front of --hnet; refine.csv lists the moved
residues, with --n_decoys every decoy is refined and ensemble.csv gains refine_moved, refine_F_before and refine_F_after.
--clashscore / --hydrogens (without them every output byte as before): --clashscore writes clashes.csv for the
written structure -- one line per serious all-atom overlap with placed hydrogens (atoms named as in hbonds.csv, distance, overlap in
A, kept | gained | lost against the input's own side chains) -- and prints the clashscore (with the input's own beside it);
--hydrogens writes structure_H.pdb, structure.pdb plus the placed hydrogens.  --hnet optimises flips and
rotatable hydrogens first: structure.pdb takes the flipped angles, structure_H.pdb the optimised hydrogens, hnet.csv lists the movers.  With --n_decoys ensemble.csv gains the columns clashscore
and clashes_interface.  --disulfides hands its bridges on: a bonded cysteine has no HG and the bridge is not an overlap.  The score
is NOT MolProbity's: this package's radius table, and flips and rotatable hydrogens only with --hnet.
--anchors auto|geometry|SPEC (without --anchors every output byte as before): behind the sampler and the
disulfide closure the side chains that coordinate a metal or are covalently linked to a ligand are closed onto it (``Context.anchors``)
and, with --use_proximal, held by the proximal stage.  Not with --n_decoys.  Writes anchors.csv (one line per anchor: residue, atom,
target, kind, d0, distance before and after, angle, E, status) and, when the hetero lines are written (--obstacles), LINK records at
the head of structure.pdb.
--disulfides auto|SPEC (without --disulfides every output byte as before): behind the sampler the chi1 of every
bonded cysteine pair are set so that the two sulfurs meet -- auto finds the pairs from the backbone, SPEC names them
('A:5-A:55,A:14-A:38').  With --use_proximal the proximal stage then keeps the bonded residues; with --repack a kept residue keeps its
chi1.  Not with --n_decoys.  Writes disulfides.csv (chain, number, partner chain, partner number, Emin, E, SG-SG distance, chi3, chi1
before, chi1 after; angles in degrees) and SSBOND records at the head of structure.pdb.
"""
import argparse
import os
from pathlib import Path

import numpy as np
import torch

from ..analysis import ProteinAnalysis
from ..functional import get_atom14_coords
from ..module import TDiffusionModule
from ..pdb_io import OBSTACLE_MODES, contains_sidechains, from_pdb_file, insert_obstacle_lines, obstacles_for, to_pdb


def load_model(args):
    from ..config import load_hot_path_configs, resolve_ckpt
    config_dir = args.config_dir or os.environ.get("PACKPPI_CONFIG_DIR")
    cfgs = load_hot_path_configs(config_dir) if config_dir else None
    cfg_kw = dict(encoder_cfg=cfgs.encoder_cfg, model_cfg=cfgs.model_cfg, sample_cfg=cfgs.sample_cfg) if cfgs else {}
    if cfgs is not None:
        print(f"----- Using the configuration tree {cfgs.config_dir} -----")
    ckpt = resolve_ckpt(args.ckpt_path, cfgs)
    if args.random_weights is not None:
        from ..weights import make_random_state_dict
        print(f"----- Using seeded random weights (seed {args.random_weights}); no checkpoint given! -----")
        model = TDiffusionModule(make_random_state_dict(args.random_weights), device=args.device, **cfg_kw)
    else:
        assert ckpt is not None and os.path.exists(ckpt), "Invalid checkpoint path!"
        print(f"----- Loading {ckpt} checkpoint! -----")
        model = TDiffusionModule.load_from_checkpoint(ckpt, map_location=args.device, strict=False, **cfg_kw)
    if args.steps is not None:
        model.schedule = torch.linspace(1, 0, args.steps + 1)
    return model.eval()


def add_guide_arguments(p):
    """--guide and its companions.  Their defaults are SUPPRESSed: without the flags the namespace is what it was before them."""
    S = argparse.SUPPRESS
    p.add_argument("--guide", type=float, default=S, metavar="SCALE", help="Clash-guided sampling (DESIGN.md section 21): the step size "
                   "of the gradient step on the clash loss (obstacle atoms included) between the network evaluations; 0.02 is the "
                   "starting value the CPU oracle suggests, not a tuned one. Writes guide.csv.")
    p.add_argument("--guide_schedule", choices=("late", "constant"), default=S, help="With --guide: nudge from --guide_from on (late, "
                   "default) or at every step (constant).")
    p.add_argument("--guide_from", type=float, default=S, metavar="T", help="With --guide_schedule late: nudge where the schedule's "
                   "time is at most T (default 0.3).")
    p.add_argument("--guide_cap", type=float, default=S, metavar="RAD", help="With --guide: the largest step of one angle at one "
                   "nudge, in radians (default 0.1).")


def guide_from_args(args, p=None):
    """The ``guide`` dict of ``TDiffusionModule.sampling`` from the command line, None without --guide."""
    given = [k for k in ("guide_schedule", "guide_from", "guide_cap") if hasattr(args, k)]
    if not hasattr(args, "guide"):
        if given and p is not None:
            p.error("--" + given[0] + " belongs to --guide")
        return None
    g = dict(scale=args.guide)
    for key, name in (("guide_schedule", "kind"), ("guide_from", "t_on"), ("guide_cap", "cap")):
        if hasattr(args, key):
            g[name] = getattr(args, key)
    if p is not None:
        if not (np.isfinite(g["scale"]) and g["scale"] >= 0):
            p.error("--guide must be a finite, non-negative step size")
        if "cap" in g and not g["cap"] > 0:
            p.error("--guide_cap must be positive")
    return g


def write_guide_csv(model, outdir):
    """guide.csv from the traces the guided runs left in ``model.guide_traces``: one line per (complex or decoy, nudge point)."""
    sched = [float(t) for t in model.schedule]
    rows, n = ["complex,nudge_point,t,eta,mean_clash"], 0
    first = last = None
    for eta, trace in model.guide_traces:
        for seg in trace.cpu().tolist():
            for j, (t, e, c) in enumerate(zip(sched, eta.tolist(), seg)):
                rows.append(f"{n},{j},{t!r},{e!r}," + ("" if c != c else repr(c)))
            traced = [c for c in seg if c == c]
            if traced and first is None:
                first = traced[0]
            if traced:
                last = traced[-1]
            n += 1
    with open(os.path.join(outdir, "guide.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")
    if first is not None:
        print(f"----- guide: mean clash in front of the first nudge {first:.4f}, in front of the last {last:.4f} -----")
    else:
        print("----- guide: no nudge ran (every eta is 0) -----")


def add_corrector_arguments(p):
    """--corrector and --corrector_from.  Their defaults are SUPPRESSed, like the guide's."""
    S = argparse.SUPPRESS
    p.add_argument("--corrector", type=float, default=S, metavar="SNR", help="Predictor-corrector sampling (DESIGN.md section 23): one "
                   "Langevin corrector of this signal-to-noise ratio behind every reverse step but the last, with a step size per "
                   "complex; 0.16 is the reference's constant (step_correct), nothing here is tuned against a trained checkpoint. "
                   "Needs --seed. Writes corrector.csv.")
    p.add_argument("--corrector_from", type=float, default=S, metavar="T", help="With --corrector: correct where the schedule's time "
                   "behind the step is at most T (default 1: everywhere).")


def corrector_from_args(args, p=None):
    """The ``corrector`` dict of ``TDiffusionModule.sampling`` from the command line, None without --corrector."""
    if not hasattr(args, "corrector"):
        if hasattr(args, "corrector_from") and p is not None:
            p.error("--corrector_from belongs to --corrector")
        return None
    c = dict(snr=args.corrector)
    if hasattr(args, "corrector_from"):
        c["t_on"] = args.corrector_from
    if p is not None:
        if not (np.isfinite(c["snr"]) and c["snr"] >= 0):
            p.error("--corrector must be a finite, non-negative signal-to-noise ratio")
        if not np.isfinite(c.get("t_on", 1.0)):
            p.error("--corrector_from must be finite")
        if getattr(args, "seed", None) is None:
            p.error("--corrector needs --seed (the corrector draws its noise from the seeded generator)")
    return c


def write_corrector_csv(model, outdir):
    """corrector.csv from ``model.corrector_traces``: one line per (reverse step, complex or decoy); empty where no corrector ran."""
    sched = [float(t) for t in model.schedule]
    rows, n = ["step,t,complex,s2,n2,eps,amp"], 0
    for _, trace in model.corrector_traces:
        for seg in trace.cpu().tolist():
            for j, vals in enumerate(seg):
                rows.append(f"{j},{sched[j + 1]!r},{n}," + ",".join("" if v != v else repr(v) for v in vals))
            n += 1
    with open(os.path.join(outdir, "corrector.csv"), "w") as fh:
        fh.write("\n".join(rows) + "\n")


def add_disulfide_arguments(p):
    """--disulfides.  Its default is SUPPRESSed, like the guide's: without the flag the namespace is what it was before it."""
    p.add_argument("--disulfides", type=str, default=argparse.SUPPRESS, metavar="auto|SPEC", help="Close disulfide bridges behind the "
                   "sampler (DESIGN.md section 26): auto detects the cysteine pairs from the backbone, SPEC names them, e.g. "
                   "'A:5-A:55,A:14-A:38' (chain and PDB residue number). With --use_proximal the proximal stage keeps the bonded "
                   "residues. Writes disulfides.csv and SSBOND records at the head of structure.pdb.")


def disulfides_from_args(args, p=None, protein=None):
    """The ``disulfides`` value of ``TDiffusionModule.sampling`` from the command line, None without --disulfides: "auto", or (with
    the parsed input) the row pairs of the residues named."""
    if not hasattr(args, "disulfides"):
        return None
    if p is not None and args.n_decoys is not None:
        p.error("--disulfides together with --n_decoys is not supported: the ensemble calls do not close bridges")
    spec = args.disulfides.strip()
    if spec == "auto" or protein is None:
        return spec
    from ..selection import parse_disulfides
    return parse_disulfides(spec, protein)


def disulfides_csv(protein, partner, report, chi_before, chi_after):
    """The text of disulfides.csv and the bonded row pairs: one line per bonded residue -- chain, number, partner chain, partner
    number, Emin, E, SG-SG distance (A), chi3, chi1 before, chi1 after (degrees) -- from host lists of ``Context.disulfides``."""
    deg = 180.0 / np.pi
    lines = ["chain,number,partner_chain,partner_number,emin,energy,sg_sg_distance,chi3,chi1_before,chi1_after\n"]
    pairs = []
    for a, b in enumerate(partner):
        if b < 0:
            continue
        if b > a:
            pairs.append((a, b))
        r = report[a]
        lines.append(f"{protein['chain_id'][a]},{int(protein['residue_index'][a])},{protein['chain_id'][b]},{int(protein['residue_index'][b])},"
                     f"{r[0]:.4f},{r[1]:.4f},{r[2]:.4f},{r[3] * deg:.2f},{chi_before[a] * deg:.2f},{chi_after[a] * deg:.2f}\n")
    return "".join(lines), pairs


def write_disulfides(model, protein, outdir):
    """disulfides.csv from the report the run left in ``model.disulfide_reports``; returns the SSBOND text of the written structure."""
    from ..pdb_io import ssbond_records
    rep = model.disulfide_reports[-1]
    if bool((rep["count"] < 0).any()):
        from ..lib import DISULFIDE_OVERFLOW
        raise RuntimeError(DISULFIDE_OVERFLOW)
    partner, report = rep["partner"].reshape(-1).cpu().tolist(), rep["report"].reshape(-1, 4).cpu().tolist()
    before, after = rep["chi_before"].reshape(-1, 4)[:, 0].cpu().tolist(), rep["chi_after"].reshape(-1, 4)[:, 0].cpu().tolist()
    text, pairs = disulfides_csv(protein, partner, report, before, after)
    with open(os.path.join(outdir, "disulfides.csv"), "w") as fh:
        fh.write(text)
    print(f"----- disulfides: {len(pairs)} bridges closed -----")
    return ssbond_records(protein, pairs, [report[a][2] for a, _ in pairs])


def add_anchor_arguments(p):
    """--anchors.  Its default is SUPPRESSed, like --disulfides: without the flag the namespace is what it was before it."""
    p.add_argument("--anchors", type=str, default=argparse.SUPPRESS, metavar="auto|geometry|SPEC", help="Close metal sites and "
                   "covalent links behind the sampler (DESIGN.md section 34): auto takes the input's LINK records between a side-chain "
                   "atom and a HETATM or non-standard-residue atom, geometry the donor atoms within reach of a metal in the input's "
                   "own coordinates (they decide which atoms coordinate, never where they go), SPEC names them, e.g. "
                   "'A:94:NE2=A:301:ZN' (chain, PDB residue number, atom). With --use_proximal the proximal stage keeps the closed "
                   "residues. Writes anchors.csv and, with --obstacles, LINK records at the head of structure.pdb.")


def anchors_from_args(args, p=None, protein=None):
    """The ``anchors`` value of ``TDiffusionModule.sampling`` from the command line, None without --anchors: "auto" (the module reads
    the LINK records of ``batch.pdb_path``), or (with the parsed input) the ``AnchorSet`` of "geometry" or of the atoms named."""
    if not hasattr(args, "anchors"):
        return None
    if p is not None and getattr(args, "n_decoys", None) is not None:
        p.error("--anchors together with --n_decoys is not supported: the ensemble calls do not close anchors")
    spec = args.anchors.strip()
    if spec == "auto" or protein is None:
        return spec
    from ..pdb_io import anchor_sites, hetero_atoms
    from ..selection import parse_anchors
    return anchor_sites(args.input, protein, "geometry", log=print) if spec == "geometry" else parse_anchors(spec, protein, hetero_atoms(args.input))


ANCHOR_STATUS = {0: "none", 1: "closed", 2: "kept", -1: "open", -2: "dropped"}


def anchors_csv(protein, anchors, status, report, anchor_report, before):
    """The text of anchors.csv: one line per anchor -- chain, number, atom, target, kind, d0, the distance before and after (A), the
    angle (degrees), the row's E at the pick and its status -- from host lists of ``Context.anchors`` (``before``: the anchors'
    reports at the angles the closure started from)."""
    from .. import constants as rc
    lines = ["chain,number,atom,target,kind,d0,distance_before,distance_after,angle,energy,status\n"]
    for i in range(len(anchors)):
        r = int(anchors.rows[i])
        atom = rc.atom14_names[int(protein["aaindex"][r])][int(anchors.slots[i])]
        target = anchors.labels[i].partition("=")[2] or "/".join(f"{v:.3f}" for v in anchors.targets[i])
        lines.append(f"{protein['chain_id'][r]},{int(protein['residue_index'][r])},{atom},{target},{anchors.kinds[i]},{anchors.params[i][0]:.3f},"
                     f"{before[i][0]:.4f},{anchor_report[i][0]:.4f},{anchor_report[i][1]:.2f},{report[r][1]:.4f},{ANCHOR_STATUS[status[r]]}\n")
    return "".join(lines)


def write_anchors(rep, ctx, protein, outdir, pdb_file, with_links):
    """anchors.csv from a report of the shape ``model.anchor_reports`` holds; returns the LINK text of the closed and kept anchors
    (``with_links``: the hetero lines are written too, so the records have both ends), else ""."""
    from ..pdb_io import hetero_atoms, link_lines
    a = rep["anchors"]
    status, report = rep["status"].reshape(-1).cpu().tolist(), rep["report"].reshape(-1, 4).cpu().tolist()
    arep = rep["anchor_report"].cpu().tolist()
    if -2 in status:
        raise RuntimeError("anchors: the device dropped an entry the host check let through")
    # the distances the closure started from: the same anchors with every row kept, at chi_before
    before = ctx.anchors(rep["chi_before"], a, fixed=np.ones(ctx.n_rows, np.uint8), check=False).anchor_report.cpu().tolist() if len(a) else []
    with open(os.path.join(outdir, "anchors.csv"), "w") as fh:
        fh.write(anchors_csv(protein, a, status, report, arep, before))
    done = [i for i in range(len(a)) if status[int(a.rows[i])] in (1, 2)]
    print(f"----- anchors: {sum(1 for v in status if v == 1)} residues closed, {sum(1 for v in status if v == -1)} left open -----")
    if not with_links or not done:
        return ""
    return link_lines(protein, a, hetero_atoms(pdb_file), [arep[i][0] for i in done], keep=done)


def write_ensemble(model, batch, protein, args, analysis):
    """--n_decoys: sample, write every decoy, the two tables and the selected decoy; returns the selected angles [1, L, 4]."""
    from .. import constants as rc
    kw = dict(recombine=True, recombine_sweeps=args.recombine_sweeps) if args.recombine else {}
    out = model.sample_ensemble(batch, args.n_decoys, seed=args.seed, use_proximal=args.use_proximal, select=args.select,
                                return_all=True, **kw, **(dict(sasa=True) if args.sasa else {}),
                                **(dict(polar=True) if getattr(args, "polar", False) else {}),
                                **(dict(clashscore=True) if getattr(args, "clashscore", False) else {}),
                                **(dict(hbond_optimize=True) if getattr(args, "hnet", False) else {}), **args.guide_kw)
    chi, packed = out["decoys"]
    best = int(out["best"][0])
    args.refine_rows = (packed.seg_offsets_host[best], best)       # --refine_allatom: the selected decoy's first row and segment
    dev, clash = out["dev"].cpu().tolist(), out["clash"].cpu().tolist()
    print(f"----- {args.n_decoys} decoys in one packed pass; selected decoy {best} ({args.select}) -----")
    xyz = get_atom14_coords(packed.X, packed.residue_type, packed.BB_D, chi).cpu().squeeze(0).numpy()
    offs = packed.seg_offsets_host
    texts = []
    for d in range(args.n_decoys):
        # pack() drops trailing rows without a residue (no backbone): they keep the input's coordinates, as they carry no side chain
        pos = np.array(protein["atom_positions"], dtype=np.float32)
        pos[:offs[d + 1] - offs[d]] = xyz[offs[d]:offs[d + 1]]
        texts.append(insert_obstacle_lines(to_pdb(dict(protein, atom_positions=pos)), args.obstacle_lines))
        with open(os.path.join(args.outdir, f"decoy_{d:03d}.pdb"), "w") as fh:
            fh.write(texts[-1])
    final = write_recombined(model, batch, protein, args, out) if args.recombine else texts[best]
    with open(analysis.tmp_pdb, "w") as fh:
        fh.write(final)
    with open(os.path.join(args.outdir, "ensemble.csv"), "w") as fh:
        bsa = out["bsa"].cpu().tolist() if args.sasa else None
        pcols = [k for k in POLAR_ENSEMBLE_COLUMNS if k in out] if getattr(args, "polar", False) else []
        pvals = [out[k].cpu().tolist() for k in pcols]
        aa = getattr(args, "clashscore", False)
        score, face = (out["clashscore"].cpu().tolist(), out["clashes_interface"].cpu().tolist()) if aa else (None, None)
        hcols = [k for k in ("hnet_bonds", "hnet_flips", "clashscore_hnet") if k in out] if getattr(args, "hnet", False) else []
        hvals = [out[k].cpu().tolist() for k in hcols]
        if "refine_moved" in out:
            hcols += ["refine_moved", "refine_F_before", "refine_F_after"]
            hvals += [out["refine_moved"].cpu().tolist(), out["refine_F"][:, 0].cpu().tolist(), out["refine_F"][:, 1].cpu().tolist()]
        fh.write("decoy,key,dev,clash,selected" + (",bsa" if args.sasa else "") + "".join("," + k for k in pcols)
                 + (",clashscore,clashes_interface" if aa else "") + "".join("," + k for k in hcols) + "\n")
        for d, key in enumerate(out["keys"]):
            fh.write(f"{d},{key},{dev[d]!r},{clash[d]!r},{int(d == best)}" + (f",{bsa[d]!r}" if args.sasa else "")
                     + "".join(f",{int(v[d])}" for v in pvals) + (f",{score[d]!r},{int(face[d])}" if aa else "")
                     + "".join(f",{v[d]!r}" if isinstance(v[d], float) else f",{int(v[d])}" for v in hvals) + "\n")
    conf = out["confidence"][0].cpu().tolist()
    conf += [[0.0] * 4] * (len(protein["aaindex"]) - len(conf))
    with open(os.path.join(args.outdir, "confidence.csv"), "w") as fh:
        fh.write("chain,residue_number,residue_name,resultant_chi1,resultant_chi2,resultant_chi3,resultant_chi4\n")
        for cid, num, aa, r in zip(protein["chain_id"], protein["residue_index"], protein["aaindex"], conf):
            fh.write(f"{cid},{int(num)},{rc.resnames[int(aa)]}," + ",".join(f"{v:.6f}" for v in r) + "\n")
    return out["recombined"] if args.recombine else out["selected"]


def write_recombined(model, batch, protein, args, out):
    """--recombine: recombined.pdb and recombine.csv from ``sample_ensemble(recombine=True, return_all=True)``; returns the text of
    recombined.pdb.  The local energies come from two more calls of the same entry without sweeps: E_r(best | all rows at best) on
    the ensemble, E_r(pick_r | the picks) on one copy of the complex at the recombined angles."""
    from .. import constants as rc
    from ..batch import replicate
    from ..functional import _ctx_for
    chi, packed = out["decoys"]
    cfg = model.hparams.sample_cfg
    clash_kw = dict(vtf=cfg.violation_tolerance_factor, tol=cfg.clash_overlap_tolerance)
    best = int(out["best"][0])
    one = replicate(batch, 1)
    before = model._context(packed).ensemble_recombine(chi, args.n_decoys, start=out["best"], max_sweeps=0, want_energy=True,
                                                       **clash_kw).energy[:, best].cpu().tolist()
    after = _ctx_for(one).ensemble_recombine(out["recombined"], 1, max_sweeps=0, want_energy=True, **clash_kw).energy[:, 0].cpu().tolist()
    pick = out["pick"].cpu().tolist()
    trace = out["clash_trace"][0].cpu().tolist()
    moved = sum(int(p != best) for p in pick)
    print(f"----- recombined per residue: {moved} of {len(pick)} residues from another decoy, {int(out['sweeps'][0])} sweeps"
          f"{'' if int(out['converged'][0]) else ' (not converged)'}, mean clash {trace[0]:.4f} -> {trace[-1]:.4f} -----")
    xyz = get_atom14_coords(one.X, one.residue_type, one.BB_D, out["recombined"]).cpu().squeeze(0).numpy()
    pos = np.array(protein["atom_positions"], dtype=np.float32)
    pos[:len(xyz)] = xyz
    text = insert_obstacle_lines(to_pdb(dict(protein, atom_positions=pos)), args.obstacle_lines)
    with open(os.path.join(args.outdir, "recombined.pdb"), "w") as fh:
        fh.write(text)
    n = len(protein["aaindex"])
    pad = n - len(pick)                   # trailing rows without a residue: not part of the ensemble, they keep the selected decoy
    with open(os.path.join(args.outdir, "recombine.csv"), "w") as fh:
        fh.write("chain,residue_number,residue_name,decoy,energy_before,energy_after\n")
        for cid, num, aa, d, e0, e1 in zip(protein["chain_id"], protein["residue_index"], protein["aaindex"], pick + [best] * pad,
                                           before + [0.0] * pad, after + [0.0] * pad):
            fh.write(f"{cid},{int(num)},{rc.resnames[int(aa)]},{d},{e0!r},{e1!r}\n")
    return text


def obstacle_share(model, batch, chi):
    """[L] the clash of every residue against the obstacles at ``chi``: Context.clash with the set minus Context.clash after
    clearing it (the set is put back)."""
    from ..functional import _ctx_for
    cfg = model.hparams.sample_cfg
    kw = dict(vtf=cfg.violation_tolerance_factor, tol=cfg.clash_overlap_tolerance)
    ctx = _ctx_for(batch)
    with_set = ctx.clash(chi, **kw)
    ctx.set_obstacles(None)
    without = ctx.clash(chi, **kw)
    ctx.set_obstacles(batch.obstacle_xyzr, ctx._obstacle_ranges(batch), polar=batch.get("obstacle_polar"))
    return (with_set - without)[0].cpu().tolist()


def write_obstacles_csv(model, batch, protein, args, chi_after):
    """obstacles.csv: residue, chain, clash against obstacles before (the input's angles) and after (the result's)."""
    before, after = obstacle_share(model, batch, batch.SC_D), obstacle_share(model, batch, chi_after)
    with open(os.path.join(args.outdir, "obstacles.csv"), "w") as fh:
        fh.write("residue,chain,clash_obstacles_before,clash_obstacles_after\n")
        for num, cid, b, a in zip(protein["residue_index"], protein["chain_id"], before, after):
            fh.write(f"{int(num)},{cid},{b!r},{a!r}\n")
    hit = sum(1 for a in after if a > 0)
    print(f"----- obstacles: clash against them {sum(before):.4f} -> {sum(after):.4f} (summed over residues; {hit} residues still touch) -----")


def write_sasa(batch, protein, outdir, chi, name="sasa.csv"):
    """--sasa: sasa.csv of the B = 1 ``batch`` at the angles ``chi`` [1, n, 4] (n < L: the trailing rows without a residue that
    pack() dropped keep the batch's angles)."""
    from ..analysis import write_sasa_csv
    from ..functional import solvent_accessibility
    chi = chi.to(batch.SC_D.device)
    if chi.shape[1] != batch.SC_D.shape[1]:
        chi = torch.cat([chi, batch.SC_D[:, chi.shape[1]:]], 1)
    write_sasa_csv(os.path.join(outdir, name), protein, solvent_accessibility(batch, chi))


POLAR_ENSEMBLE_COLUMNS = ("hbonds", "hbonds_interface", "salt_interface", "buns_interface")


def write_polar(batch, protein, outdir, chi, sasa=False, native=False, names=("polar.csv", "hbonds.csv")):
    """--polar: polar.csv and hbonds.csv of the B = 1 ``batch`` at the angles ``chi`` [1, n, 4] (n < L: as in ``write_sasa``), and
    the summary line.  ``sasa``: polar.csv gains the column buns.  ``native``: the input has side chains of its own -- hbonds.csv
    marks every bond kept, gained or lost against them and the summary gives the recovery.  The polar obstacle atoms are the
    batch's (``obstacle_polar``), as in the ensemble columns.  ``names``: the two file names."""
    from ..analysis import hbonds_csv_text, polar_csv_text
    from ..functional import _ctx_for, polar_contacts, polar_recovery
    chi = chi.to(batch.SC_D.device)
    if chi.shape[1] != batch.SC_D.shape[1]:
        chi = torch.cat([chi, batch.SC_D[:, chi.shape[1]:]], 1)
    res = polar_contacts(batch, chi, sasa=sasa)
    ref = polar_contacts(batch) if native else None
    xyz = _ctx_for(batch).atom14(chi)[0].cpu().numpy()
    with open(os.path.join(outdir, names[0]), "w") as fh:
        fh.write(polar_csv_text(protein, res.res[0].cpu().numpy(), res.buns[0].cpu().numpy() if sasa else None))
    with open(os.path.join(outdir, names[1]), "w") as fh:
        fh.write(hbonds_csv_text(protein, xyz, res.partners[0].cpu().numpy(), ref.partners[0].cpu().numpy() if native else None))
    seg = res.seg[0].cpu().tolist()
    line = (f"----- polar: {seg[0]} hydrogen bonds, {seg[1]} between chains, {seg[5]} salt bridges between chains, "
            f"{seg[7]} polar atoms without a partner")
    if sasa:
        line += f", {int(res.buns.sum())} of them buried ({int(res.buns_interface.sum())} by the interface)"
    if native:
        n, k = polar_recovery(ref, res)
        line += f"; recovered {int(k[0])} of {int(n[0])} native side-chain hydrogen bonds"
    print(line + " -----")


def add_allatom_arguments(p):
    """--clashscore and --hydrogens.  Their defaults are SUPPRESSed: without the flags the namespace is what it was before them."""
    p.add_argument("--clashscore", action="store_true", default=argparse.SUPPRESS, help="Write clashes.csv for the written structure "
                   "(DESIGN.md section 29): every serious all-atom overlap with hydrogens placed on the device, and print the "
                   "clashscore (overlaps per 1000 atoms; NOT MolProbity's number: flips and rotatable hydrogens only with --hnet, "
                   "this package's radii); with --n_decoys ensemble.csv gains the columns clashscore and clashes_interface.")
    p.add_argument("--hydrogens", action="store_true", default=argparse.SUPPRESS, help="Write structure_H.pdb: the records of the "
                   "written structure plus the hydrogens placed on the device behind each residue's heavy atoms (DESIGN.md section 29; "
                   "hydroxyl, thiol and lysine NH3+ hydrogens at a conventional position, not an optimised one; --hnet optimises them).")
    p.add_argument("--hnet", action="store_true", default=argparse.SUPPRESS, help="Optimise the hydrogen-bond network of the written "
                   "structure on the device (DESIGN.md section 30): Asn / Gln / His flips and the rotatable hydrogens of Ser, Thr, Tyr, "
                   "Cys and Lys.  structure.pdb takes the flipped angles, structure_H.pdb (--hydrogens) the optimised hydrogens, hnet.csv "
                   "holds one line per mover, and the --clashscore summary gains the score with the rotatable hydrogens counted, before "
                   "and after.  Integer counts of overlaps and bonds, not Reduce's dot scores.")
    p.add_argument("--refine_allatom", action="store_true", default=argparse.SUPPRESS, help="Refine the side chains in chi space against "
                   "the explicit-hydrogen overlaps --clashscore counts, on the device (DESIGN.md section 32), behind the proximal stage and "
                   "the disulfide closure and in front of --hnet: small steps on one chi at a time, a residue without a serious overlap "
                   "keeps its angles.  structure.pdb takes the refined angles, refine.csv holds one line per moved residue, the "
                   "--clashscore summary gains the score before and after, and with --n_decoys ensemble.csv gains refine_moved, "
                   "refine_F_before and refine_F_after.  Kept rows (--repack) and bonded cysteines stay.  Step sizes and bands are "
                   "starting values, not tuned ones.")


def optimise_hnet(batch, protein, outdir, chi, link=None, name="hnet.csv"):
    """--hnet: ``Context.hbond_optimize`` of the B = 1 ``batch`` at the angles ``chi`` [1, n, 4] (n < L: as in ``write_sasa``), hnet.csv and
    the summary line.  Returns the result; its ``chi`` [1, L, 4] holds the flips."""
    from ..analysis import write_hnet
    from ..functional import _ctx_for
    chi = chi.to(batch.SC_D.device)
    if chi.shape[1] != batch.SC_D.shape[1]:
        chi = torch.cat([chi, batch.SC_D[:, chi.shape[1]:]], 1)
    res = _ctx_for(batch).hbond_optimize(chi=chi, link=link)
    write_hnet(os.path.join(outdir, name), protein, res, 0)
    return res


def write_allatom(batch, protein, outdir, chi, clashscore=False, hydrogens=False, native=False, link=None, head="", obstacle_lines=(),
                  names=("clashes.csv", "structure_H.pdb"), hnet=None, unrefined=None):
    """--clashscore / --hydrogens: clashes.csv and structure_H.pdb of the B = 1 ``batch`` at the angles ``chi`` [1, n, 4] (n < L: as in
    ``write_sasa``), and the summary line.  ``native``: the input has side chains of its own -- clashes.csv marks every overlap kept,
    gained or lost against them and the summary gives the input's own score.  ``link``: the partner array of the run's disulfide
    closure.  ``head`` / ``obstacle_lines``: what the written structure carries around its ATOM records.  ``hnet``: what
    ``optimise_hnet`` returned for ``chi`` before its flips went into it -- structure_H.pdb then takes the optimised hydrogens, and the
    summary gains the score with the rotatable hydrogens counted, conventional and optimised.  ``unrefined``: the angles [1, n, 4]
    --refine_allatom started from -- the summary gains the score before and after it."""
    from ..analysis import write_clashes, write_structure_h
    from ..functional import _ctx_for
    chi = chi.to(batch.SC_D.device)
    if chi.shape[1] != batch.SC_D.shape[1]:
        chi = torch.cat([chi, batch.SC_D[:, chi.shape[1]:]], 1)
    ctx = _ctx_for(batch)
    if clashscore:
        h = ctx.clashscore(chi=chi, link=link)
        write_clashes(os.path.join(outdir, names[0]), protein, h, 0, ctx.clashscore(link=link) if native else None)
        if unrefined is not None:
            was = unrefined.to(batch.SC_D.device)
            if was.shape[1] != batch.SC_D.shape[1]:
                was = torch.cat([was, batch.SC_D[:, was.shape[1]:]], 1)
            before = ctx.clashscore(chi=was, link=link, want_partners=False)
            after = h if hnet is None else ctx.clashscore(chi=hnet.chi0, link=link, want_partners=False)
            print(f"----- clashscore {float(before.clashscore[0]):.2f} before, {float(after.clashscore[0]):.2f} after the all-atom "
                  f"refinement (--refine_allatom) -----")
        if hnet is not None:
            conv = ctx.clashscore(chi=hnet.chi0, link=link, rotatable="keep", want_partners=False)
            opt = ctx.clashscore(chi=hnet.chi, link=link, hydrogens=hnet, rotatable="keep", want_partners=False)
            print(f"----- clashscore with the rotatable hydrogens counted: {float(conv.clashscore[0]):.2f} as placed, "
                  f"{float(opt.clashscore[0]):.2f} with the hydrogen-bond network optimised (--hnet) -----")
    else:
        h = ctx.hydrogens(chi=chi, link=link)
    if hnet is not None:
        h = hnet
    if hydrogens:
        n = len(protein["aaindex"])
        placed = dict(protein, atom_positions=h.xyz[0].reshape(-1, 14, 3)[:n].cpu().numpy())
        write_structure_h(os.path.join(outdir, names[1]), placed, h, 0, head, obstacle_lines)


def evaluate_model(model, args):
    print("----- Starting evaluation! -----")
    analysis = ProteinAnalysis(args.molprobity_clash_loc, args.outdir, args.device)
    protein = from_pdb_file(Path(args.input), mse_to_met=True)
    obstacles = obstacles_for(args.input, args.obstacles)
    args.obstacle_lines = obstacles["lines"] if obstacles else []
    batch = analysis.get_prot(args.input)
    if obstacles is not None:
        from ..featurize import _add_obstacles
        _add_obstacles(batch, obstacles)
    batch = batch.to(args.device)
    if args.seed is not None:
        torch.manual_seed(args.seed)
    # --seed: the initial noise and the sde noise come from the counter-based device generator (module.sampling(seed=...)): the
    # same seed gives the same structure on any device, shard layout and torch version
    guide = guide_from_args(args)
    args.guide_kw = dict(guide=guide) if guide is not None else {}
    model.keep_guide_trace = guide is not None
    corrector = corrector_from_args(args)
    if corrector is not None:
        args.guide_kw["corrector"] = corrector
    model.keep_corrector_trace = corrector is not None
    disulfides = disulfides_from_args(args, protein=protein)
    if disulfides is not None:
        from ..selection import residue_names
        args.guide_kw["disulfides"] = disulfides
        batch["residue_names"] = residue_names(protein)        # so that a refusal names the residue, not the row
    model.keep_disulfide_report = disulfides is not None
    anchors = anchors_from_args(args, protein=protein)
    if anchors is not None:
        from ..selection import residue_names
        args.guide_kw["anchors"] = anchors
        batch["residue_names"], batch["pdb_path"] = residue_names(protein), args.input
        model.keep_anchor_report, model.anchor_reports = True, []
    refine_on = getattr(args, "refine_allatom", False)
    if refine_on:
        args.guide_kw["refine_allatom"] = True
        model.keep_refine_report, model.refine_reports = True, []
    fixed = None
    if args.repack is not None:
        from ..selection import device_selector, interface_selection, parse_selection, sasa_selection
        kind = device_selector(args.repack, args.obstacles)
        if kind is not None:
            sel = sasa_selection(batch, kind)
        else:
            sel = interface_selection(protein, args.input) if args.repack == "interface" else parse_selection(args.repack, protein)
        print(f"----- Repacking {int(sel.sum())} of {len(sel)} residues ({args.fixed_mode}); the others keep the input's angles -----")
        fixed = torch.from_numpy(~sel).unsqueeze(0)
    if args.n_decoys is not None:
        SC_D_sample = write_ensemble(model, batch, protein, args, analysis)
    elif fixed is not None:
        SC_D_sample = model.repack(batch, fixed, seed=args.seed, fixed_mode=args.fixed_mode, use_proximal=args.use_proximal,
                                   **args.guide_kw)
    else:
        SC_D_sample = model.sampling(batch, use_proximal=args.use_proximal, seed=args.seed, **args.guide_kw)
    if guide is not None:
        write_guide_csv(model, args.outdir)
    if corrector is not None:
        write_corrector_csv(model, args.outdir)
    ssbond = write_disulfides(model, protein, args.outdir) if disulfides is not None else ""
    if anchors is not None:            # LINK records behind the SSBOND records, as in a deposited file
        ssbond += write_anchors(model.anchor_reports[-1], model._context(batch), protein, args.outdir, args.input, bool(args.obstacle_lines))
    if model.saturated() & 4:
        print("----- WARNING: NaN / infinity in the input coordinates or angles: the reference would return NaN here -----")
    if model.saturated() & 3:
        # a hidden activation reached the f16 maximum in the split-f16 dense layers: not the reference's arithmetic any more
        print("----- WARNING: f16 saturation in the score network (flag %d); run `python -m packppi_amd.rangecheck` on this "
              "checkpoint -----" % model.saturated())
    unrefined = None
    if refine_on:
        from ..analysis import write_refine
        rep = model.refine_reports[-1]
        first = args.refine_rows[0] if args.n_decoys is not None else 0
        unrefined = rep.chi0.reshape(1, -1, 4)[:, first:first + SC_D_sample.shape[1]]
        write_refine(os.path.join(args.outdir, "refine.csv"), protein, rep, args.refine_rows[1] if args.n_decoys is not None else 0, first)
    hnet = None
    if getattr(args, "hnet", False):
        # with --n_decoys structure.pdb stays the selected decoy's file; hnet.csv and structure_H.pdb describe its optimised network
        link = model.disulfide_reports[-1]["partner"] if disulfides is not None else None
        hnet = optimise_hnet(batch, protein, args.outdir, SC_D_sample, link)
        if args.n_decoys is None:
            SC_D_sample = hnet.chi[:, :SC_D_sample.shape[1]].to(SC_D_sample.device)
    if args.n_decoys is None:           # --n_decoys wrote structure.pdb itself: byte for byte the selected decoy's file
        xyz = get_atom14_coords(batch.X, batch.residue_type, batch.BB_D, SC_D_sample)
        protein["atom_positions"] = xyz.cpu().squeeze(0).numpy()
        with open(analysis.tmp_pdb, "w") as fh:
            fh.writelines(ssbond + insert_obstacle_lines(to_pdb(protein), args.obstacle_lines))
    if obstacles is not None:
        write_obstacles_csv(model, batch, protein, args, SC_D_sample)
    if args.sasa:
        write_sasa(batch, protein, args.outdir, SC_D_sample)
    if getattr(args, "polar", False):
        write_polar(batch, protein, args.outdir, SC_D_sample, sasa=args.sasa, native=contains_sidechains(args.input))
    if getattr(args, "clashscore", False) or getattr(args, "hydrogens", False):
        link = model.disulfide_reports[-1]["partner"] if disulfides is not None else None
        write_allatom(batch, protein, args.outdir, SC_D_sample, getattr(args, "clashscore", False), getattr(args, "hydrogens", False),
                      native=contains_sidechains(args.input), link=link, head=ssbond, obstacle_lines=args.obstacle_lines,
                      **(dict(hnet=hnet) if hnet is not None else {}), **(dict(unrefined=unrefined) if unrefined is not None else {}))
    if contains_sidechains(args.input):
        metric = analysis.get_metric(true_pdb=args.input, pred_pdb=analysis.tmp_pdb)
        print(f"----- Metric: ----- {metric}")
    else:
        print("----- No side chain atoms found in the input PDB. Skipping metric calculation. -----")
    print("----- Finishing evaluation! -----")


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--input", type=str, help="The input pdb file path.", required=True)
    p.add_argument("--outdir", type=str, help="Directory to store outputs.", required=True)
    p.add_argument("--molprobity_clash_loc", type=str, help="Path to /build/bin/molprobity.clashscore.", required=True)
    p.add_argument("--use_proximal", action="store_true", help="Use proximal optimize.")
    p.add_argument("--device", type=str, help="cuda (the MI355X HIP device)", default="cuda")
    p.add_argument("--ckpt_path", type=str, default=None, help="Lightning checkpoint (else $PACKPPI_CKPT, else the config tree's ckpt_path).")
    p.add_argument("--config_dir", type=str, default=None, help="The reference's configs/ directory (else $PACKPPI_CONFIG_DIR): "
                   "encoder / model / sampling YAML files are read from it.")
    p.add_argument("--steps", type=int, default=None, help="Diffusion steps (reference schedule: 30).")
    p.add_argument("--seed", type=int, default=None, help="Seed of the sampling noise (initial and sde), drawn by the "
                   "counter-based generator on the device; default: unseeded draws from torch's generator.")
    p.add_argument("--random_weights", type=int, default=None, help="Seeded stand-in weights instead of a checkpoint.")
    p.add_argument("--repack", type=str, default=None, metavar="SPEC|interface", help="Repack only these residues, e.g. "
                   "'A:45-60,B:12,C' (chain and PDB residue number) or 'interface'; the others keep the input's angles. Needs --seed.")
    p.add_argument("--fixed_mode", choices=("hold", "renoise"), default="renoise", help="With --repack: what the kept residues look "
                   "like to the network during sampling: re-noised to each step's level (renoise) or clean throughout (hold).")
    p.add_argument("--n_decoys", type=int, default=None, metavar="D", help="Draw D seeded decoys in one packed pass; writes "
                   "decoy_000.pdb ..., structure.pdb (the selected decoy), ensemble.csv and confidence.csv. Needs --seed.")
    p.add_argument("--select", choices=("clash", "medoid"), default="clash", help="With --n_decoys: keep the decoy with the lowest "
                   "mean clash (clash) or the one closest to the circular consensus (medoid).")
    p.add_argument("--recombine", action="store_true", help="With --n_decoys: recombine the decoys per residue by clash descent from "
                   "the selected one; writes recombined.pdb and recombine.csv, and structure.pdb is the recombined structure.")
    p.add_argument("--recombine_sweeps", type=int, default=64, metavar="K", help="With --recombine: the largest number of sweeps.")
    p.add_argument("--obstacles", choices=OBSTACLE_MODES, default="none", help="Fixed atoms the clash stages keep the side chains off (DESIGN.md section 19): none (default), hetero = every HETATM record and "
                   "every non-standard residue (ligands, cofactors, nucleic acids; no hydrogens, waters or metals), hetero+water = the "
                   "waters too. The diffusion network does not see them: sampling is unchanged, the clash stages (--use_proximal, "
                   "decoy ranking, --recombine) repair what it puts into the pocket. Written structures keep the records.")
    p.add_argument("--sasa", action="store_true", help="Write sasa.csv for the written structure (DESIGN.md section 20): per residue "
                   "the solvent-accessible area next to itself alone, in its isolated chain, in the complex and with the obstacle "
                   "atoms, the buried interface area and the exposure; with --n_decoys ensemble.csv gains the column bsa. "
                   "--repack also takes interface:sasa (the delta-SASA interface of the input, made on the device) and pocket "
                   "(residues whose surface the obstacle atoms bury; needs --obstacles).")
    p.add_argument("--polar", action="store_true", default=argparse.SUPPRESS, help="Write polar.csv (per residue: hydrogen-bond "
                   "partners of side-chain and backbone atoms within and between chains, salt-bridge partner residues, polar "
                   "obstacle contacts, polar atoms without a partner; with --sasa the buried ones, buns) and hbonds.csv (every "
                   "hydrogen bond between chains or with a side-chain atom, kept | gained | lost against the input's own side "
                   "chains) for the written structure (DESIGN.md section 27); with --n_decoys ensemble.csv gains the columns "
                   "hbonds, hbonds_interface, salt_interface and, with --sasa, buns_interface.")
    add_guide_arguments(p)
    add_corrector_arguments(p)
    add_disulfide_arguments(p)
    add_anchor_arguments(p)
    add_allatom_arguments(p)
    return p


def parse_args(argv=None):
    p = build_parser()
    args = p.parse_args(argv)
    try:
        from ..selection import device_selector
        device_selector(args.repack, args.obstacles)
    except ValueError as e:
        p.error(str(e))
    if args.repack is not None and args.seed is None:
        p.error("--repack needs --seed (the kept residues are re-noised with the seeded generator's draws)")
    if args.n_decoys is not None:
        if args.seed is None:
            p.error("--n_decoys needs --seed (unseeded noise is laid out over the whole batch: a decoy would depend on its place in it)")
        if args.n_decoys < 1:
            p.error("--n_decoys must be at least 1")
        if args.repack is not None:
            p.error("--n_decoys together with --repack is not supported: ensembles under a fixed mask are not implemented")
    if args.recombine and args.n_decoys is None:
        p.error("--recombine needs --n_decoys (it recombines the decoys of an ensemble)")
    if args.recombine_sweeps < 0:
        p.error("--recombine_sweeps must not be negative")
    guide_from_args(args, p)
    corrector_from_args(args, p)
    disulfides_from_args(args, p)
    anchors_from_args(args, p)
    return args


def main(argv=None):
    args = parse_args(argv)
    evaluate_model(load_model(args), args)


if __name__ == "__main__":
    main()
