"""``ProteinAnalysis``: PDB -> batch, metrics and MolProbity clashscore around the sampler.

Mirrors src/utils/protein_analysis.py: ``get_prot`` (:103-122), ``get_metric`` (:36-91), ``compute_rmsd``
(:93-101), ``get_clashscore`` (:26-34).  ``run_tool`` (SCWRL/FASPR/Rosetta wrappers) is out of scope.
Interface residues (src/utils/interface.py:11-56: any atom within 10 A of an atom of another chain) are found
with a KD-tree instead of Biopython's NeighborSearch; like the PDB reader this step is parity-unpinned.
"""
import os
import subprocess
from pathlib import Path

import numpy as np
import torch

from .featurize import chain_numbers_and_offset_index, protein_to_batch
from .functional import get_atom14_coords
from .pdb_io import from_pdb_file


def interface_residues(pdb_file, radius=10.0):
    """{chain: sorted residue numbers having an atom within ``radius`` of another protein chain} or None."""
    from scipy.spatial import cKDTree
    xyz, chain, resseq, is_std = [], [], [], {}
    with open(pdb_file) as fh:
        for ln in fh:
            if ln.startswith("ENDMDL"):
                break
            if not ln.startswith(("ATOM", "HETATM")):
                continue
            try:
                p = (float(ln[30:38]), float(ln[38:46]), float(ln[46:54]))
                rs = int(ln[22:26])
            except ValueError:
                continue
            c = ln[21]
            xyz.append(p); chain.append(c); resseq.append(rs)
            is_std[c] = is_std.get(c, False) or ln.startswith("ATOM")
    chains = [c for c, ok in is_std.items() if ok]
    if len(chains) < 2:
        return None
    keep = np.array([c in chains for c in chain])
    xyz, chain, resseq = np.array(xyz)[keep], np.array(chain)[keep], np.array(resseq)[keep]
    tree = cKDTree(xyz)
    pairs = tree.query_pairs(radius, output_type="ndarray")
    cross = chain[pairs[:, 0]] != chain[pairs[:, 1]]
    out = {c: set() for c in chains}
    for side in (0, 1):
        idx = pairs[cross, side]
        for c in chains:
            out[c].update(resseq[idx[chain[idx] == c]].tolist())
    return {c: sorted(v) for c, v in out.items()}


def interface_mask(protein, pdb, radius=10.0):
    """helper.py:104-128."""
    if len(np.unique(protein["chain_id"])) == 1:
        return None
    inter = interface_residues(pdb, radius)
    if inter is None:
        return None
    parts = []
    for cid in np.unique(protein["chain_id"]):
        sub = protein["residue_index"][protein["chain_id"] == cid]
        parts.append(np.isin(sub, inter[cid]) if cid in inter else np.zeros(len(sub), bool))
    return torch.from_numpy(np.concatenate(parts)).float()


def sphere_points(n_points):
    """The test points of ``Context.sasa``: ``n_points`` unit vectors on the golden spiral, float32 [P, 3].
    Computed in float64 -- z_k = 1 - (2k + 1) / P, phi_k = k pi (3 - sqrt 5), (sqrt(1 - z^2) cos phi, sqrt(1 - z^2) sin phi, z) --
    and rounded to float32 once: deterministic, the same table on every host."""
    P = int(n_points)
    if P < 1:
        raise ValueError(f"n_points must be at least 1, got {n_points}")
    k = np.arange(P, dtype=np.float64)
    z = 1.0 - (2.0 * k + 1.0) / P
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    s = np.sqrt(1.0 - z * z)
    return np.ascontiguousarray(np.stack([s * np.cos(phi), s * np.sin(phi), z], 1).astype(np.float32))


SASA_CSV_HEADER = "chain,number,name,sasa_residue,sasa_chain,sasa_complex,sasa_ligand,bsa,exposure"


def sasa_csv_text(protein, area, bsa, exposure):
    """The text of ``sasa.csv``: one line per residue of ``protein`` -- chain, residue number, residue name, the four areas of
    ``Context.sasa`` in A^2 (next to the own residue alone, in the isolated chain, in the complex, with the obstacle atoms), the
    buried interface area and the exposure.  ``area`` [n, 4], ``bsa`` / ``exposure`` [n] (lists or arrays); rows of ``protein``
    beyond n (trailing rows without a residue) get zeros."""
    from . import constants as rc
    area, bsa, exposure = np.asarray(area, dtype=np.float64).reshape(-1, 4), np.asarray(bsa, dtype=np.float64), np.asarray(exposure, dtype=np.float64)
    lines = [SASA_CSV_HEADER]
    for r, (cid, num, aa) in enumerate(zip(protein["chain_id"], protein["residue_index"], protein["aaindex"])):
        a, b, e = (area[r], bsa[r], exposure[r]) if r < len(area) else (np.zeros(4), 0.0, 0.0)
        lines.append(f"{cid},{int(num)},{rc.resnames[int(aa)]}," + ",".join(f"{v:.3f}" for v in a) + f",{b:.3f},{e:.4f}")
    return "\n".join(lines) + "\n"


def write_sasa_csv(path, protein, res, row=0):
    """``sasa.csv`` at ``path`` from what ``Context.sasa`` returned for a B = 1 batch of ``protein``; prints the summary line."""
    area = res.area[row].cpu().numpy()
    with open(path, "w") as fh:
        fh.write(sasa_csv_text(protein, area, res.bsa[row].cpu().numpy(), res.exposure[row].cpu().numpy()))
    seg = res.seg_area[row].cpu().tolist()
    print(f"----- sasa: {seg[2]:.1f} A^2 accessible in the complex, {seg[1] - seg[2]:.1f} A^2 buried between chains, "
          f"{seg[2] - seg[3]:.1f} A^2 buried by obstacle atoms; {int(res.interface[row].sum())} interface residues -----")


POLAR_CSV_HEADER = ("chain,number,name,hb_side_same,hb_side_other,hb_back_same,hb_back_other,salt_same,salt_other,"
                    "obstacle_partners,unsatisfied")
HBONDS_CSV_HEADER = "chain_a,number_a,name_a,atom_a,chain_b,number_b,name_b,atom_b,distance,status"


def obstacle_polar(obstacles):
    """uint8 [M]: 1 for the atoms of ``pdb_io.obstacle_atoms`` output whose element is N or O (``constants.obstacle_polar_elements``),
    what ``Context.polar(obst_polar=...)`` takes; None for None."""
    from . import constants as rc
    if obstacles is None:
        return None
    return np.array([1 if str(e).upper() in rc.obstacle_polar_elements else 0 for e in obstacles["element"]], dtype=np.uint8)


def polar_csv_text(protein, res, buns=None):
    """The text of ``polar.csv``: one line per residue of ``protein`` -- chain, residue number, residue name and the eight ``res``
    columns of ``Context.polar`` ([n, 8]); with ``buns`` ([n, 14] bool, or [n] counts) one more column, the buried unsatisfied polar
    atoms of the residue.  Rows of ``protein`` beyond n get zeros."""
    from . import constants as rc
    res = np.asarray(res, dtype=np.int64).reshape(-1, 8)
    if buns is not None:
        buns = np.asarray(buns)
        buns = buns.reshape(len(buns), -1).astype(np.int64).sum(1)
    lines = [POLAR_CSV_HEADER + (",buns" if buns is not None else "")]
    for r, (cid, num, aa) in enumerate(zip(protein["chain_id"], protein["residue_index"], protein["aaindex"])):
        v = res[r] if r < len(res) else np.zeros(8, np.int64)
        tail = "" if buns is None else f",{int(buns[r]) if r < len(buns) else 0}"
        lines.append(f"{cid},{int(num)},{rc.resnames[int(aa)]}," + ",".join(str(int(x)) for x in v) + tail)
    return "\n".join(lines) + "\n"


def polar_bonds(partners):
    """The hydrogen bonds behind the ``partners`` array of ONE segment ([n, 14, 4] integers, on the host) as a sorted list of
    ((row, slot), (row, slot)) with the lower code first: a bond is listed when either atom lists the other."""
    p = np.asarray(partners).reshape(-1, 14, np.asarray(partners).shape[-1])
    out = set()
    for r, s, k in zip(*np.nonzero(p >= 0)):
        a, b = int(r) * 14 + int(s), int(p[r, s, k])
        out.add((min(a, b), max(a, b)))
    return [(divmod(a, 14), divmod(b, 14)) for a, b in sorted(out)]


def hbonds_csv_text(protein, xyz, partners, native_partners=None):
    """The text of ``hbonds.csv`` for ONE complex: one line per hydrogen bond between chains or with a side-chain atom (slot >= 4) --
    chain, number, residue name and atom name on both sides, the distance in A at ``xyz`` [n, 14, 3] and, against
    ``native_partners`` (the bonds of the input's own side chains), ``kept`` (in both), ``gained`` (only here) or ``lost`` (only
    there; the distance is then that at ``xyz`` too); without ``native_partners`` the status is empty."""
    from . import constants as rc
    xyz = np.asarray(xyz, dtype=np.float64).reshape(-1, 14, 3)
    chain, num, aa = list(protein["chain_id"]), list(protein["residue_index"]), list(protein["aaindex"])

    def wanted(bond):
        (ra, sa), (rb, sb) = bond
        return chain[ra] != chain[rb] or sa >= 4 or sb >= 4

    here = [b for b in polar_bonds(partners) if wanted(b)]
    rows = [(b, "") for b in here]
    if native_partners is not None:
        there = set(b for b in polar_bonds(native_partners) if wanted(b))
        rows = [(b, "kept" if b in there else "gained") for b in here] + [(b, "lost") for b in sorted(there - set(here))]
        rows.sort(key=lambda t: t[0])
    lines = [HBONDS_CSV_HEADER]
    for ((ra, sa), (rb, sb)), status in rows:
        d = float(np.linalg.norm(xyz[ra, sa] - xyz[rb, sb]))
        side = lambda r, s: f"{chain[r]},{int(num[r])},{rc.resnames[int(aa[r])]},{rc.atom14_names[int(aa[r])][s]}"
        lines.append(f"{side(ra, sa)},{side(rb, sb)},{d:.3f},{status}")
    return "\n".join(lines) + "\n"


CLASHES_CSV_HEADER = "chain_a,number_a,name_a,atom_a,chain_b,number_b,name_b,atom_b,distance,overlap,status"


def clash_pairs(partners):
    """The serious overlaps behind the ``partners`` array of ONE segment of ``Context.clashscore`` ([n, 27, 4] integers, on the host)
    as a sorted list of ((row, slot), (row, slot)), lower code first: a pair is listed when either atom lists the other (an atom
    with more than four partners lists its lowest four)."""
    p = np.asarray(partners)
    p = p.reshape(-1, 27, p.shape[-1])
    out = set()
    for r, s, k in zip(*np.nonzero(p >= 0)):
        a, b = int(r) * 27 + int(s), int(p[r, s, k])
        out.add((min(a, b), max(a, b)))
    return [(divmod(a, 27), divmod(b, 27)) for a, b in sorted(out)]


def clashes_csv_text(protein, xyz, hxyz, partners, radius, hb_allow=0.6, native_partners=None):
    """The text of ``clashes.csv`` for ONE complex: one line per serious overlap of ``Context.clashscore`` --
    chain, number, residue name and atom name on both sides (hydrogens by their PDB v3 names), the distance in A and the overlap
    (rx + ry - d, less ``hb_allow`` between a polar hydrogen and an acceptor; ``radius`` [n, 27] as the call counted them), computed
    here in float64, and, against ``native_partners`` (the overlaps of the input's own side chains), ``kept``, ``gained`` or
    ``lost`` (distance and overlap are then those at ``xyz`` too); without ``native_partners`` the status is empty."""
    from . import constants as rc
    pos = np.concatenate([np.asarray(xyz, dtype=np.float64).reshape(-1, 14, 3), np.asarray(hxyz, dtype=np.float64).reshape(-1, 13, 3)], 1)
    radius = np.asarray(radius, dtype=np.float64).reshape(-1, 27)
    chain, num, aa = list(protein["chain_id"]), list(protein["residue_index"]), list(protein["aaindex"])
    here = clash_pairs(partners)
    rows = [(b, "") for b in here]
    if native_partners is not None:
        there = set(clash_pairs(native_partners))
        rows = [(b, "kept" if b in there else "gained") for b in here] + [(b, "lost") for b in sorted(there - set(here))]
        rows.sort(key=lambda t: t[0])
    lines = [CLASHES_CSV_HEADER]
    for ((ra, sa), (rb, sb)), status in rows:
        d = float(np.linalg.norm(pos[ra, sa] - pos[rb, sb]))
        ca, cb = int(rc.allatom_class[int(aa[ra]), sa]), int(rc.allatom_class[int(aa[rb]), sb])
        pair = ((ca & rc.AA_POLAR_H) and (cb & rc.AA_ACCEPTOR)) or ((ca & rc.AA_ACCEPTOR) and (cb & rc.AA_POLAR_H))
        ov = radius[ra, sa] + radius[rb, sb] - (float(hb_allow) if pair else 0.0) - d
        side = lambda r, s: f"{chain[r]},{int(num[r])},{rc.resnames[int(aa[r])]},{rc.allatom_names[int(aa[r])][s]}"
        lines.append(f"{side(ra, sa)},{side(rb, sb)},{d:.3f},{ov:.3f},{status}")
    return "\n".join(lines) + "\n"


def clashscore_summary(res, row=0, native=None):
    """The summary line of the command lines for segment ``row`` of a ``Context.clashscore`` result (``native``: that of the input's
    own side chains, reported beside it)."""
    seg = res.seg[row].cpu().tolist()
    line = (f"----- clashscore (all atoms, placed hydrogens; not MolProbity): {float(res.clashscore[row]):.2f}, {seg[1]} serious overlaps, "
            f"{seg[2]} between chains, {seg[7]} backbone only")
    if native is not None:
        line += f"; the input's own side chains: {float(native.clashscore[row]):.2f}"
    return line + " -----"


def write_clashes(path, protein, res, row=0, native=None, hb_allow=0.6):
    """``clashes.csv`` at ``path`` from what ``Context.clashscore`` returned for a B = 1 batch of ``protein``; prints the summary."""
    n = len(protein["aaindex"])
    cut = lambda t, *shape: t[row].reshape(-1, *shape)[:n].cpu().numpy()
    with open(path, "w") as fh:
        fh.write(clashes_csv_text(protein, cut(res.xyz, 14, 3), cut(res.hxyz, 13, 3), cut(res.partners, 27, 4),
                                  res.radius.reshape(res.hmask.shape[0], -1, 27)[row][:n].cpu().numpy(), hb_allow,
                                  cut(native.partners, 27, 4) if native is not None else None))
    print(clashscore_summary(res, row, native))


HNET_CSV_HEADER = "chain,residue,name,kind,state,angle,e_before,e_after"


def hnet_csv(residue_type, state, e, chain, residue_index):
    """The text of ``hnet.csv``: one line per mover (``state`` >= 0) of what ``Context.hbond_optimize`` returned -- chain, residue
    number, residue name, kind (rotor / flip), the chosen state, its angle in degrees (the dihedral of a rotor's first hydrogen; 0 or
    180 for a flip) and the row's energy before and after.  All arguments per row, lists or arrays; ``e`` [n, 2]."""
    from . import constants as rc
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    lines = [HNET_CSV_HEADER]
    for r, (aa, st) in enumerate(zip(residue_type, state)):
        if int(st) < 0:
            continue
        kind = {rc.MOVER_ROTOR: "rotor", rc.MOVER_FLIP: "flip"}[int(rc.mover_table[int(aa), 0])]
        lines.append(f"{chain[r]},{int(residue_index[r])},{rc.resnames[int(aa)]},{kind},{int(st)},{rc.mover_state_angle(int(aa), int(st)):.1f},"
                     f"{int(e[r, 0])},{int(e[r, 1])}")
    return "\n".join(lines) + "\n"


REFINE_CSV_HEADER = "chain,residue,name,steps_chi1,steps_chi2,steps_chi3,steps_chi4,rotation_deg,e_before,e_after"


def refine_csv(residue_type, steps, deltas_deg, e, chain, residue_index):
    """The text of ``refine.csv``: one line per residue ``Context.refine_allatom`` moved -- chain, residue number, residue name, the
    steps taken on each chi as ``round1/round2/...`` (a step of round r is ``deltas_deg[r]`` degrees), the total rotation in degrees
    (the sum of |steps| x delta over rounds and angles) and the row's energy before and after.  ``steps`` [rounds, n, 4], ``e`` [n, 2]."""
    from . import constants as rc
    steps = np.asarray(steps, dtype=np.int64).reshape(len(deltas_deg), -1, 4)
    e = np.asarray(e, dtype=np.int64).reshape(-1, 2)
    lines = [REFINE_CSV_HEADER]
    for r, aa in enumerate(residue_type):
        if r >= steps.shape[1] or not steps[:, r].any():
            continue
        cols = ["/".join(str(int(v)) for v in steps[:, r, j]) for j in range(4)]
        rot = sum(abs(int(v)) * float(d) for d, row in zip(deltas_deg, steps[:, r]) for v in row)
        lines.append(f"{chain[r]},{int(residue_index[r])},{rc.resnames[int(aa)]},{','.join(cols)},{rot:.1f},{int(e[r, 0])},{int(e[r, 1])}")
    return "\n".join(lines) + "\n"


def refine_summary(res, row=0):
    """The summary line of the command lines for segment ``row`` of a ``Context.refine_allatom`` result."""
    lo_hi = res.F[row].cpu().tolist()
    return (f"----- all-atom refinement: energy {lo_hi[0]} -> {lo_hi[1]}, sweeps per round {res.sweeps[:, row].cpu().tolist()}"
            f"{'' if bool(res.converged[:, row].all()) else ' (not converged)'} -----")


def write_refine(path, protein, res, seg=0, first_row=0):
    """``refine.csv`` at ``path`` from what ``Context.refine_allatom`` returned: the rows of ``protein`` are rows ``first_row`` ... of the
    result (0 for a B = 1 batch; a decoy's first row in a packed one) and ``seg`` is their segment; prints the summary."""
    n = len(protein["aaindex"])
    R = res.steps.shape[0]
    steps = res.steps.reshape(R, -1, 4)[:, first_row:first_row + n].cpu().numpy()
    steps = np.concatenate([steps, np.zeros((R, n - steps.shape[1], 4), steps.dtype)], 1)     # trailing rows a packed batch dropped
    e = res.e.reshape(-1, 2)[first_row:first_row + n].cpu().numpy()
    e = np.concatenate([e, np.zeros((n - e.shape[0], 2), e.dtype)], 0)
    with open(path, "w") as fh:
        fh.write(refine_csv(protein["aaindex"], steps, [float(np.rad2deg(d)) for d in res.deltas], e, protein["chain_id"],
                            protein["residue_index"]))
    print(refine_summary(res, seg))


def hnet_summary(res, row=0):
    """The summary line of the command lines for segment ``row`` of a ``Context.hbond_optimize`` result."""
    st = res.state.reshape(-1)
    tr = res.trace[row].cpu().tolist()
    return (f"----- hydrogen-bond network: {int(res.n_movers[row])} movers, energy {tr[0]} -> {tr[-1]} in {int(res.sweeps[row])} sweeps"
            f"{'' if int(res.converged[row]) else ' (not converged)'} -----")


def write_hnet(path, protein, res, row=0):
    """``hnet.csv`` at ``path`` from what ``Context.hbond_optimize`` returned for a B = 1 batch of ``protein``; prints the summary."""
    n = len(protein["aaindex"])
    with open(path, "w") as fh:
        fh.write(hnet_csv(protein["aaindex"], res.state[row].reshape(-1)[:n].cpu().numpy(), res.e[row].reshape(-1, 2)[:n].cpu().numpy(),
                          protein["chain_id"], protein["residue_index"]))
    print(hnet_summary(res, row))


def write_structure_h(path, protein, h, row=0, head="", obstacle_lines=()):
    """``structure_H.pdb`` at ``path``: ``pdb_io.to_pdb_hydrogens`` of ``protein`` with the hydrogens ``Context.hydrogens`` (or
    ``clashscore``) placed for a B = 1 batch of it; ``head``: records that go in front (SSBOND); ``obstacle_lines``: the obstacle
    records, kept as in structure.pdb."""
    from .pdb_io import insert_obstacle_lines, to_pdb_hydrogens
    n = len(protein["aaindex"])
    text = to_pdb_hydrogens(protein, h.hxyz[row].reshape(-1, 13, 3)[:n].cpu().numpy(), h.hmask[row].reshape(-1, 13)[:n].cpu().numpy())
    with open(path, "w") as fh:
        fh.write(head + insert_obstacle_lines(text, list(obstacle_lines)))


class ProteinAnalysis:
    def __init__(self, molprobity_clash_loc, tmp_dir, device="cuda", device_clashscore=False):
        """``device_clashscore``: ``get_metric`` also returns ``clashscore_device``, the all-atom clashscore of the predicted structure
        with hydrogens placed on the device (``functional.clashscore``; not MolProbity's number).  Off by
        default: the dict and its ``clashscore`` entry are then exactly what they were."""
        self.molprobity_clash_loc = molprobity_clash_loc
        self.device_clashscore = bool(device_clashscore)
        self.device = device
        self.tmp_dir = tmp_dir
        os.makedirs(self.tmp_dir, exist_ok=True)
        self.tmp_log = os.path.join(tmp_dir, "molprobity_clash.log")
        self.tmp_pdb = os.path.join(tmp_dir, "structure.pdb")

    def get_clashscore(self, pdb):
        """External MolProbity binary; returns None when it is unavailable or prints no score."""
        if not self.molprobity_clash_loc or not os.path.exists(str(self.molprobity_clash_loc).split()[0]):
            return None
        cmd = f"{self.molprobity_clash_loc} model={pdb} keep_hydrogens=True > {self.tmp_log}"
        subprocess.run(cmd, shell=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        try:
            with open(self.tmp_log) as fh:
                for ln in fh:
                    if "clashscore" in ln and "= " in ln:
                        txt = ln.split("= ")[1].strip()
                        return float(txt) if txt.replace(".", "").isdigit() else None
        except OSError:
            pass
        return None

    def get_prot(self, pdb, get_interface=True):
        protein = from_pdb_file(Path(pdb), mse_to_met=True)
        data = protein_to_batch(protein)
        if get_interface:
            # Reference behaviour kept: prot_to_data shifts the residue numbers of every chain after the first IN PLACE in the
            # protein dict it is given (complex_dataset.py:79,91: torch.from_numpy(...).to(int64) shares memory with the
            # int64 array the PDB reader returns), and get_interface_mask, called after it (protein_analysis.py:106-108),
            # compares those shifted numbers with the file's own numbering -- so only residues of the first chain (and
            # accidental number matches) can enter the interface mask, and interface_acc is an accuracy over them.
            shifted = dict(protein, residue_index=chain_numbers_and_offset_index(protein)[1].numpy())
            im = interface_mask(shifted, pdb)
            rm = data.residue_mask[0]
            data["interface_mask"] = ((im * rm) if im is not None else torch.zeros_like(rm)).unsqueeze(0)
        return data

    def compute_rmsd(self, true_coords, pred_coords, atom_mask, residue_mask, eps=1e-6):
        w = atom_mask * residue_mask[..., None]
        return (torch.sum((true_coords - pred_coords) ** 2, dim=-1) * w).sum() / (w + eps).sum()

    def get_metric(self, true_pdb, pred_pdb):
        try:
            true_data = self.get_prot(true_pdb, get_interface=True)
            pred_data = self.get_prot(pred_pdb)
        except Exception as e:  # noqa: BLE001  (the reference reports and returns None)
            print(f"Error: Failed to load or parse PDB files. Details: {str(e)}")
            return None
        if true_data.X.shape[1] != pred_data.X.shape[1]:
            print("Error: Mismatch in the number of residues between true and predicted structures.")
            return None
        clashscore = self.get_clashscore(pred_pdb)
        imask = true_data.interface_mask
        ct, cp, cm, pi1 = true_data.SC_D, pred_data.SC_D, true_data.SC_D_mask, true_data.chi_1pi_periodic_mask
        metric, total_acc, interface_acc = {}, 0, 0
        for i in range(4):
            n = cm[..., i].sum()
            n = n if n != 0 else 1
            ni = (cm[..., i] * imask).sum()
            ni = ni if ni != 0 else 1
            diff = (cp[..., i] - ct[..., i]).abs()
            acc = torch.logical_and(diff * 180 / np.pi < 20, diff > 0).float()
            ae = torch.minimum(diff, 2 * np.pi - diff)
            ae = torch.where(pi1[..., i], torch.minimum(ae, np.pi - ae), ae)
            metric[f"chi_{i}_ae_rad"] = ae.sum() / n
            metric[f"chi_{i}_ae_deg"] = (ae * 180 / np.pi).sum() / n
            metric[f"chi_{i}_acc"] = acc.sum() / n
            total_acc += acc.sum() / n
            interface_acc += (acc * imask).sum() / ni
        d = torch.device(self.device)
        pred_xyz = get_atom14_coords(true_data.X.to(d), true_data.residue_type.to(d), true_data.BB_D.to(d),
                                     pred_data.SC_D.to(d)).cpu()
        metric["atom_rmsd"] = self.compute_rmsd(true_data.X, pred_xyz, true_data.atom_mask, true_data.residue_mask)
        metric["total_acc"] = total_acc / 4
        metric["interface_acc"] = interface_acc / 4
        metric["clashscore"] = clashscore
        if self.device_clashscore:
            from .functional import clashscore as device_clashscore
            metric["clashscore_device"] = float(device_clashscore(pred_data.to(d), want_partners=False).clashscore[0])
        return metric
