"""Protein dict -> batch tensors (host side, torch CPU).

Mirrors what ``ComplexDataset.prot_to_data`` (complex_dataset.py:65-148) and the dihedral
helpers (helper.py:20-101) compute, so that a batch built here is interchangeable with
the reference's.  SURVEY.md §8(f) row 1.
"""
from typing import Dict

import numpy as np
import torch
import torch.nn.functional as F

from . import constants as rc
from .batch import Batch, as_single


def _unit(v: torch.Tensor) -> torch.Tensor:
    return torch.nan_to_num(v / torch.norm(v, dim=-1, keepdim=True))


def dihedrals_along(points: torch.Tensor) -> torch.Tensor:
    """Signed dihedral of every 4 consecutive points along axis -2 (helper.py:20-36)."""
    bond = _unit(points[..., 1:, :] - points[..., :-1, :])
    b_prev, b_mid, b_next = bond[..., :-2, :], bond[..., 1:-1, :], bond[..., 2:, :]
    n_a = _unit(torch.cross(b_prev, b_mid, dim=-1))
    n_b = _unit(torch.cross(b_mid, b_next, dim=-1))
    cosang = torch.clamp((n_a * n_b).sum(-1), -1 + 1e-8, 1 - 1e-8)
    return torch.sign((b_prev * n_b).sum(-1)) * torch.acos(cosang)


def backbone_dihedrals(X: torch.Tensor, residue_index: torch.Tensor):
    """(pre-omega, phi, psi) per residue and their validity mask (helper.py:39-74)."""
    L = X.shape[0]
    chain = X[:, :3].reshape(3 * L, 3)
    d = F.pad(dihedrals_along(chain), [1, 2], value=float("nan")).reshape(L, 3)   # phi, psi, omega
    nan1 = torch.tensor([float("nan")])
    zero1 = torch.tensor([0.0])
    follows_prev = torch.cat((zero1, (residue_index[1:] - 1 == residue_index[:-1]).float()))
    precedes_next = torch.cat(((residue_index[:-1] + 1 == residue_index[1:]).float(), zero1))
    pre_omega = torch.cat((nan1, d[:-1, 2]))
    bb = torch.stack((pre_omega, d[:, 0], d[:, 1]), dim=-1)
    mask = torch.stack((follows_prev, follows_prev, precedes_next), dim=-1)
    mask = mask * torch.isfinite(bb).float()
    return bb, mask


def sidechain_dihedrals(X: torch.Tensor, aatype: torch.Tensor):
    """chi1..chi4 from atom14 coordinates and their mask (helper.py:77-101)."""
    idx = torch.from_numpy(rc.chi_atom_indices_atom14)[aatype]                    # [L,7]
    cmask = torch.from_numpy(rc.chi_mask_atom14)[aatype]                          # [L,4]
    pts = torch.gather(X, -2, idx[..., None].expand(*idx.shape, 3))
    chi = torch.nan_to_num(dihedrals_along(pts)) * cmask
    return chi, (chi != 0.0).float()


def chain_numbers_and_offset_index(protein: Dict):
    """(chain number 1.. in order of first appearance, residue_index with every later chain pushed +100 past the already
    shifted end of the previous one) -- complex_dataset.py:80-93.  The protein dict is left untouched."""
    L = len(protein["aaindex"])
    rindex = torch.from_numpy(np.asarray(protein["residue_index"])).long().clone()
    seen = {}
    chain_np = np.empty(L, np.int64)
    for i, c in enumerate(list(protein["chain_id"])):
        chain_np[i] = seen.setdefault(c, len(seen) + 1)
    chain = torch.from_numpy(chain_np)
    if len(seen) > 1:
        shift = 0
        for c in range(1, len(seen)):
            shift += int(rindex[chain == c].max()) + 100
            rindex[chain == c + 1] += shift
    return chain, rindex


def _add_obstacles(data: Batch, obstacles) -> Batch:
    """Store obstacle atoms (``pdb_io.obstacle_atoms`` output, or any dict with ``xyz`` [M, 3] and ``radius`` [M]; None = none) in
    per-complex data as ``obstacle_xyzr`` [M, 4] float32 and ``obstacle_offsets`` [2] (batch.OBSTACLE_KEYS).  Obstacles that come
    with their ``element`` list also give ``obstacle_polar`` uint8 [M] (``analysis.obstacle_polar``: 1 for N and O), the atoms
    ``Context.polar`` counts as partners; nothing else reads it."""
    if obstacles is None:
        return data
    xyz = torch.as_tensor(np.asarray(obstacles["xyz"], np.float32)).reshape(-1, 3)
    rad = torch.as_tensor(np.asarray(obstacles["radius"], np.float32)).reshape(-1)
    if xyz.shape[0] != rad.shape[0]:
        raise ValueError(f"obstacles: {xyz.shape[0]} positions, {rad.shape[0]} radii")
    if not bool(torch.isfinite(xyz).all()) or not bool(torch.isfinite(rad).all()) or bool((rad < 0).any()):
        raise ValueError("obstacles: coordinates and radii must be finite, radii not negative")
    M = int(xyz.shape[0])
    data["obstacle_xyzr"] = torch.cat((xyz, rad[:, None]), 1).contiguous()
    data["obstacle_offsets"] = torch.tensor([0, M], dtype=torch.int32)
    data["obstacle_offsets_host"] = [0, M]
    if obstacles.get("element") is not None:
        from .analysis import obstacle_polar
        polar = torch.from_numpy(obstacle_polar(obstacles)).reshape(-1)
        if polar.shape[0] != M:
            raise ValueError(f"obstacles: {M} positions, {polar.shape[0]} elements")
        data["obstacle_polar"] = polar
    return data


def protein_to_data(protein: Dict, obstacles=None) -> Batch:
    """Per-complex tensors (no batch axis), as ``prot_to_data`` lays them out.  ``obstacles``: see ``protein_to_batch``."""
    X = torch.from_numpy(np.asarray(protein["atom_positions"])).float()
    L = X.shape[0]
    rtype = torch.from_numpy(np.asarray(protein["aaindex"])).long()
    amask = torch.from_numpy(np.asarray(protein["atom_mask"])).float()
    chain, rindex = chain_numbers_and_offset_index(protein)

    rmask = torch.isfinite(X[:, :4].sum(dim=(-1, -2))).float()
    bb, bb_mask = backbone_dihedrals(X, rindex)
    sc, sc_mask = sidechain_dihedrals(X, rtype)
    bb_sc = torch.stack((bb.sin(), bb.cos()), -1) * bb_mask[..., None]
    sc_sc = torch.stack((sc.sin(), sc.cos()), -1) * sc_mask[..., None]
    pi1 = torch.from_numpy(rc.chi_pi_periodic)[rtype].bool()
    pi2 = ~pi1

    m1, m2, m3 = rmask, rmask[:, None], rmask[:, None, None]
    sc_mask = sc_mask * m2
    data = Batch(
        num_nodes=L,
        X=X * m3,
        atom_mask=amask * m2,
        residue_type=(rtype * m1).long(),
        residue_mask=rmask,
        residue_index=(rindex * m1).long(),
        chain_indices=(chain * m1).long(),
        BB_D=bb * m2,
        BB_D_sincos=bb_sc * m3,
        BB_D_mask=bb_mask * m2,
        SC_D=sc * m2,
        SC_D_sincos=sc_sc * m3,
        SC_D_mask=sc_mask,
        chi_1pi_periodic_mask=torch.logical_and(sc_mask, pi1 * m2),
        chi_2pi_periodic_mask=torch.logical_and(sc_mask, pi2 * m2),
    )
    data.apply(lambda v: torch.nan_to_num(v) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
    return _add_obstacles(data, obstacles)


def protein_to_batch(protein: Dict, obstacles=None) -> Batch:
    """B=1 batch, the form ``ProteinAnalysis.get_prot`` hands to ``sampling`` (protein_analysis.py:103-122).

    ``obstacles`` (``pdb_io.obstacle_atoms(pdb_file)``, or None): fixed atoms -- ligands, cofactors, nucleic acids -- that every
    clash stage keeps the side chains off.  The batch then carries ``obstacle_xyzr`` and
    ``obstacle_offsets``; without them it has exactly the keys it has always had.  The network does not see obstacles."""
    return as_single(protein_to_data(protein, obstacles))


# ---- PackPPI-AP: wild type + mutant featurisation ------------------------------------------------------------------------

def parse_mutstr(mutstr: str):
    """"RA47A,EA48A" -> [{'wt': 'R', 'chain': 'A', 'resseq': 47, 'mt': 'A'}, ...] (eval_affinity.py:45-56)."""
    muts = []
    for name in mutstr.split(","):
        muts.append({"wt": name[0], "mt": name[-1], "chain": name[1], "resseq": int(name[2:-1])})
    return muts


def resolve_mutations(protein: Dict, mutations, log=print):
    """The lookup of ``mutant_data`` (skempi_dataset.py:150-185), shared with ``mutant_model_data``: [(row mask [L] bool, mutant
    residue type, tag)] of the mutations that apply, in order.  A mutation is looked up by chain and the RAW PDB residue number; one
    whose chain is absent or whose target is not one of the 20 types is skipped with the reference's message; one that matches no
    or several residues, or whose wild-type letter disagrees with the structure, raises ValueError."""
    rtype = torch.from_numpy(np.asarray(protein["aaindex"])).long()
    raw_index = np.asarray(protein["residue_index"]).astype(np.int64)
    chain_id = np.asarray(protein["chain_id"])
    path = protein.get("pdb_path")
    out = []
    for m in mutations:
        tag = f"{m['wt']}{m['chain']}{m['resseq']}{m['mt']}"
        if m["chain"] not in chain_id or m["mt"] not in rc.restypes:
            log(f"Ignore the mutation: {tag}")
            continue
        index = torch.from_numpy((chain_id == m["chain"]) & (raw_index == int(m["resseq"])))
        hits = int(index.sum())
        if hits != 1:
            raise ValueError(f"The mutation: {tag} matches {hits} residues of chain {m['chain']} in {path} file")
        ref_wt = rc.restypes[int(rtype[index])]
        if ref_wt != m["wt"]:
            raise ValueError(f"The mutation: {tag} is inconsistent with wild-type {ref_wt} in {path} file")
        out.append((index, rc.restype_order[m["mt"]], tag))
    return out


def mutant_data(protein: Dict, mutations=None, ddg=None, log=print, obstacles=None) -> Batch:
    """Per-complex wild-type and mutant tensors, as ``SkempiDataset.prot_to_data`` lays them out without ESM
    (skempi_dataset.py:73-262): the keys of ``protein_to_data`` plus ``ddg``, ``mut_mask`` and the ``*_mut`` keys.

    ``mutations`` (default ``protein['mutations']``) are dicts as ``parse_mutstr`` returns them.  A mutation is looked up
    by chain and the RAW PDB residue number (before the chain offset); one whose chain is absent or whose target residue
    is not one of the 20 types is skipped with the reference's message; a wild-type letter that disagrees with the
    structure raises ValueError.  Differences from ``protein_to_data`` that the reference makes here: the backbone dihedral
    mask is computed from the raw residue numbers, and ``SC_D_mask_mut`` from the wild-type atoms at the mutant's chi atom
    slots (it can be 1 on a mutated row while ``SC_D_mut`` and ``SC_D_sincos_mut`` are 0 there)."""
    if mutations is None:
        mutations = protein.get("mutations", [])
    X = torch.from_numpy(np.asarray(protein["atom_positions"])).float()
    L = X.shape[0]
    rtype = torch.from_numpy(np.asarray(protein["aaindex"])).long()
    amask = torch.from_numpy(np.asarray(protein["atom_mask"])).float()
    raw_index = torch.from_numpy(np.asarray(protein["residue_index"])).long()
    if ddg is None:
        ddg = protein.get("ddG", 0.0)
    ddg = torch.tensor(ddg, dtype=torch.float32)
    chain, rindex = chain_numbers_and_offset_index(protein)

    rmask = torch.isfinite(X[:, :4].sum(dim=(-1, -2))).float()
    bb, bb_mask = backbone_dihedrals(X, raw_index)
    sc, sc_mask = sidechain_dihedrals(X, rtype)
    bb_sc = torch.stack((bb.sin(), bb.cos()), -1) * bb_mask[..., None]
    sc_sc = torch.stack((sc.sin(), sc.cos()), -1) * sc_mask[..., None]
    pi1 = torch.from_numpy(rc.chi_pi_periodic)[rtype].bool()

    rtype_mut, amask_mut, sc_mut, sc_sc_mut = rtype.clone(), amask.clone(), sc.clone(), sc_sc.clone()
    for index, mt, _ in resolve_mutations(protein, mutations, log):
        rtype_mut[index] = mt
        amask_mut[index] = torch.tensor([1.0 if a else 0.0 for a in rc.atom14_names[mt]], dtype=torch.float32)
        sc_mut[index] = 0.0
        sc_sc_mut[index] = 0.0
    _, sc_mask_mut = sidechain_dihedrals(X, rtype_mut)
    pi1_mut = torch.from_numpy(rc.chi_pi_periodic)[rtype_mut].bool()
    mut_mask = (rtype != rtype_mut).long()

    m1, m2, m3 = rmask, rmask[:, None], rmask[:, None, None]
    sc_mask, sc_mask_mut = sc_mask * m2, sc_mask_mut * m2
    data = Batch(
        num_nodes=L,
        ddg=ddg,
        mut_mask=(mut_mask * m1).long(),
        X=X * m3,
        residue_mask=rmask,
        residue_index=(rindex * m1).long(),
        chain_indices=(chain * m1).long(),
        BB_D=bb * m2,
        BB_D_sincos=bb_sc * m3,
        BB_D_mask=bb_mask * m2,
        atom_mask=amask * m2,
        residue_type=(rtype * m1).long(),
        SC_D=sc * m2,
        SC_D_sincos=sc_sc * m3,
        SC_D_mask=sc_mask,
        chi_1pi_periodic_mask=torch.logical_and(sc_mask, pi1 * m2),
        chi_2pi_periodic_mask=torch.logical_and(sc_mask, ~pi1 * m2),
        atom_mask_mut=amask_mut * m2,
        residue_type_mut=(rtype_mut * m1).long(),
        SC_D_mut=sc_mut * m2,
        SC_D_sincos_mut=sc_sc_mut * m3,
        SC_D_mask_mut=sc_mask_mut,
        chi_1pi_periodic_mask_mut=torch.logical_and(sc_mask_mut, pi1_mut * m2),
        chi_2pi_periodic_mask_mut=torch.logical_and(sc_mask_mut, ~pi1_mut * m2),
    )
    data.apply(lambda v: torch.nan_to_num(v) if isinstance(v, torch.Tensor) and v.is_floating_point() else v)
    return _add_obstacles(data, obstacles)


def mutant_batch(protein: Dict, mutstr: str, log=print) -> Batch:
    """B = 1 batch of one mutation string, as eval_affinity.py:45-73 builds it (``ddg`` of shape [1])."""
    return as_single(mutant_data(protein, parse_mutstr(mutstr), log=log))


# ---- the mutant as a sampling input -----------------------------------------------------------------------

def mutant_model_data(protein: Dict, mutations=None, log=print, obstacles=None) -> Batch:
    """The mutant as a batch the sampler can pack: ``protein_to_data`` with the mutated rows rewritten for their NEW residue type.
    ``mutant_data`` builds the mutant the way PackPPI-AP consumes it (chi mask from the wild-type atoms, zero angles); this one
    builds it for ``TDiffusionModule.repack`` / ``mutate``.  Lookup, skipping and errors are ``mutant_data``'s (``resolve_mutations``).

    Every row no mutation names carries exactly what ``protein_to_data`` gives it.  A mutated row gets the new ``residue_type``,
    ``atom_mask`` from the new type's atom14 table, ``SC_D`` = ``SC_D_sincos`` = 0, ``SC_D_mask`` = the new type's chi table x
    ``residue_mask`` (not the wild-type atoms), the periodic masks from ``chi_pi_periodic`` of the new type, and X with the
    backbone slots 0-3 kept and the side-chain slots 4-13 zeroed: the old side chain is out of the way, ``atom14`` rebuilds the new
    one from the backbone frame.  The batch also carries ``mut_mask`` (int64 [L], 1 on every row a mutation that applied names --
    also one to the residue's own type: that row is rebuilt and resampled like the others) and ``mutation_tag`` (the applied tags,
    comma-separated)."""
    if mutations is None:
        mutations = protein.get("mutations", [])
    data = protein_to_data(protein, obstacles)
    for k in ("X", "atom_mask", "residue_type", "SC_D", "SC_D_sincos", "SC_D_mask", "chi_1pi_periodic_mask", "chi_2pi_periodic_mask"):
        data[k] = data[k].clone()
    rmask = data["residue_mask"]
    mut_mask = torch.zeros(int(data["num_nodes"]), dtype=torch.int64)
    chi_table, pi_table = torch.from_numpy(rc.chi_mask_atom14).float(), torch.from_numpy(rc.chi_pi_periodic).bool()
    atom_table = torch.from_numpy(np.asarray(rc.atom14_mask)).float()
    tags = []
    for index, mt, tag in resolve_mutations(protein, mutations, log):
        m1 = rmask[index]                                               # [1]
        sc_mask = chi_table[mt][None] * m1[:, None]
        data["residue_type"][index] = (mt * m1).long()
        data["atom_mask"][index] = atom_table[mt][None] * m1[:, None]
        data["SC_D"][index] = 0.0
        data["SC_D_sincos"][index] = 0.0
        data["SC_D_mask"][index] = sc_mask
        data["chi_1pi_periodic_mask"][index] = torch.logical_and(sc_mask, pi_table[mt][None])
        data["chi_2pi_periodic_mask"][index] = torch.logical_and(sc_mask, ~pi_table[mt][None])
        X = data["X"][index]
        X[:, 4:] = 0.0
        data["X"][index] = X
        mut_mask[index] = 1
        tags.append(tag)
    data["mut_mask"] = mut_mask
    data["mutation_tag"] = ",".join(tags)
    return data


def mutant_model_batch(protein: Dict, mutstr: str, log=print, obstacles=None) -> Batch:
    """B = 1 batch of ``mutant_model_data`` for one mutation string ("RA47A,EA48A"); ``obstacles`` as in ``protein_to_batch``."""
    return as_single(mutant_model_data(protein, parse_mutstr(mutstr), log=log, obstacles=obstacles))
