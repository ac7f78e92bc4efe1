"""Residue-chemistry data tables for the sampling / proximal path.

The numbers live in ``data/residue_constants.npz`` (AlphaFold2 rigid-group geometry and
Engh-Huber bond statistics, dumped from the tables the reference builds at
``src/utils/residue_constants.py:29-240,280-285,459-554,595-677,709-806`` by
``tools/oracle/make_constants.py``).  This module only loads them and derives the
parameterised distance bounds the clash loss needs.
"""
import os
from functools import lru_cache

import numpy as np

_DATA = os.path.join(os.path.dirname(__file__), "data", "residue_constants.npz")
_z = np.load(_DATA)

restypes = [str(x) for x in _z["restypes"]]                     # 20 one-letter codes
resnames = [str(x) for x in _z["resnames"]]                     # 20 three-letter + "UNK"
restype_order = {r: i for i, r in enumerate(restypes)}
resname_to_idx = {r: i for i, r in enumerate(resnames)}
atom14_names = [[str(a) for a in row] for row in _z["atom14_names"]]   # [21][14], "" = empty
sidechain_atoms = set(str(a) for a in _z["sidechain_atoms"])

default_frames = _z["default_frames"]            # [21,8,4,4] f32   rigid-group default frames
atom14_to_group = _z["atom14_to_group"]          # [21,14]    i64   rigid group of each atom14 slot
atom14_mask = _z["atom14_mask"]                  # [21,14]    f32   slot exists for the residue type
lit_positions = _z["lit_positions"]              # [21,14,3]  f32   literature position in its group
chi_angles_mask = _z["chi_angles_mask"]          # [21,4]     f32
chi_pi_periodic = _z["chi_pi_periodic"]          # [21,4]     f32
chi_atom_indices_atom14 = _z["chi_atom_indices_atom14"]   # [21,7] i64
chi_mask_atom14 = _z["chi_mask_atom14"]          # [21,4]     f32
bond_rows = _z["bond_rows"]                      # [n,5] f64  (restype, a, b, length, stddev)
slot_radius = _z["slot_radius"]                  # [21,14] f64 element vdW radius, 0 for empty slot
between_radius = _z["between_radius"]            # [21,14] f64 radius table of clash.py:263-287

# van der Waals radii by element: the four the reference's clash loss knows (residue_constants.py:280-285, what slot_radius and
# between_radius above are made of) ...
van_der_waals_radius = {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}
# ... and, for obstacle atoms (pdb_io.obstacle_atoms), Bondi's values (J. Phys. Chem. 68, 441, 1964) for the
# other elements of common ligands, cofactors and nucleic acids.  Metals are left out on purpose: an ion coordinates side chains at
# 2.0-2.3 A, which is not a clash.
obstacle_radius = dict(van_der_waals_radius, P=1.80, F=1.47, CL=1.75, BR=1.85, I=1.98, SE=1.90)

# Polar atoms (pp_polar), written out by atom name.  Class bits: 1 donor, 2 acceptor, 4 cation, 8 anion.  The
# backbone N (except proline's) donates, the backbone O accepts; the side-chain atoms are listed per residue.  An antecedent is a
# heavy atom covalently bonded to the polar atom within the residue: one or two per atom, also named here.
POLAR_DONOR, POLAR_ACCEPTOR, POLAR_CATION, POLAR_ANION = 1, 2, 4, 8
polar_donors = {"ARG": ("NE", "NH1", "NH2"), "ASN": ("ND2",), "GLN": ("NE2",), "HIS": ("ND1", "NE2"), "LYS": ("NZ",), "SER": ("OG",),
                "THR": ("OG1",), "TYR": ("OH",), "TRP": ("NE1",)}
polar_acceptors = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2"), "ASN": ("OD1",), "GLN": ("OE1",), "HIS": ("ND1", "NE2"),
                   "SER": ("OG",), "THR": ("OG1",), "TYR": ("OH",)}
polar_cations = {"LYS": ("NZ",), "ARG": ("NE", "NH1", "NH2")}
polar_anions = {"ASP": ("OD1", "OD2"), "GLU": ("OE1", "OE2")}
polar_antecedent_names = {
    "ARG": {"NE": ("CD", "CZ"), "NH1": ("CZ",), "NH2": ("CZ",)}, "ASN": {"OD1": ("CG",), "ND2": ("CG",)},
    "ASP": {"OD1": ("CG",), "OD2": ("CG",)}, "GLN": {"OE1": ("CD",), "NE2": ("CD",)}, "GLU": {"OE1": ("CD",), "OE2": ("CD",)},
    "HIS": {"ND1": ("CG", "CE1"), "NE2": ("CD2", "CE1")}, "LYS": {"NZ": ("CE",)}, "SER": {"OG": ("CB",)}, "THR": {"OG1": ("CB",)},
    "TRP": {"NE1": ("CD1", "CE2")}, "TYR": {"OH": ("CZ",)}}
obstacle_polar_elements = ("N", "O")          # the obstacle atoms pp_polar counts as partners


def _polar_tables():
    cls = np.zeros((21, 14), np.uint8)
    ante = -np.ones((21, 14, 2), np.int8)
    for t in range(20):
        names, rn = atom14_names[t], resnames[t]
        for s, nm in enumerate(names):
            if not nm:
                continue
            c, an = 0, ()
            if nm == "N" and rn != "PRO":
                c, an = POLAR_DONOR, ("CA",)
            elif nm == "O":
                c, an = POLAR_ACCEPTOR, ("C",)
            else:
                c = ((POLAR_DONOR if nm in polar_donors.get(rn, ()) else 0) | (POLAR_ACCEPTOR if nm in polar_acceptors.get(rn, ()) else 0)
                     | (POLAR_CATION if nm in polar_cations.get(rn, ()) else 0) | (POLAR_ANION if nm in polar_anions.get(rn, ()) else 0))
                if c:
                    an = polar_antecedent_names[rn][nm]
            cls[t, s] = c
            for k, a in enumerate(an):
                ante[t, s, k] = names.index(a)
    return cls, ante


polar_class, polar_antecedent = _polar_tables()   # [21,14] u8 class bits, [21,14,2] i8 antecedent slots (-1 = none)


@lru_cache(maxsize=16)
def make_atom14_dists_bounds(overlap_tolerance: float = 1.5,
                             bond_length_tolerance_factor: float = 15.0):
    """Per-residue-type lower/upper bounds on intra-residue atom distances.

    Same result as the reference's ``make_atom14_dists_bounds``
    (residue_constants.py:809-869): every existing atom pair gets
    ``lower = r_a + r_b - overlap_tolerance`` and ``upper = 1e10``; bonded and
    angle-related ("virtual bond") pairs are then overwritten with
    ``length -/+ factor * stddev``.  Arithmetic in float64, stored float32.
    """
    lower = np.zeros((21, 14, 14), np.float32)
    upper = np.zeros((21, 14, 14), np.float32)
    exists = slot_radius > 0
    for rt in range(20):
        ex = exists[rt]
        pair = ex[:, None] & ex[None, :] & ~np.eye(14, dtype=bool)
        lo = slot_radius[rt][:, None] + slot_radius[rt][None, :] - overlap_tolerance
        lower[rt][pair] = lo[pair]
        upper[rt][pair] = 1e10
    for rt, a, b, length, sd in bond_rows:
        rt, a, b = int(rt), int(a), int(b)
        lo = length - bond_length_tolerance_factor * sd
        up = length + bond_length_tolerance_factor * sd
        lower[rt, a, b] = lower[rt, b, a] = lo
        upper[rt, a, b] = upper[rt, b, a] = up
    return lower, upper
