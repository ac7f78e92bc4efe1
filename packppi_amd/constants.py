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


# Anchors: metal sites and covalent links (pp_anchor_close).  Starting values from textbook coordination
# geometry, not tuned against anything and not taken from a library: ideal donor-metal distances by donor element with the few
# metal-specific exceptions every inorganic text lists, single-bond covalent radii (Cordero et al., Dalton Trans. 2008, rounded), and
# the angle antecedent-donor-target with its tolerance per donor atom.
metal_elements = ("LI", "NA", "MG", "K", "CA", "MN", "FE", "CO", "NI", "CU", "ZN", "MO", "CD", "HG")
metal_donor_default = {"N": 2.1, "O": 2.1, "S": 2.3}                      # A, by donor element
metal_donor_distance = {("CA", "O"): 2.4, ("NA", "O"): 2.4, ("K", "O"): 2.8}   # (metal, donor element) where it differs
covalent_radius = {"C": 0.76, "N": 0.71, "O": 0.66, "S": 1.05, "P": 1.07, "F": 0.57, "CL": 1.02, "BR": 1.20, "I": 1.39, "SE": 1.20,
                   "B": 0.84, "SI": 1.11}
anchor_angle = {"HIS": {"ND1": (126.0, 15.0), "NE2": (126.0, 15.0)}, "ASP": {"OD1": (120.0, 20.0), "OD2": (120.0, 20.0)},
                "GLU": {"OE1": (120.0, 20.0), "OE2": (120.0, 20.0)}, "CYS": {"SG": (105.0, 12.0)}, "MET": {"SD": (110.0, 15.0)},
                "SER": {"OG": (115.0, 15.0)}, "THR": {"OG1": (115.0, 15.0)}, "TYR": {"OH": (115.0, 15.0)}, "LYS": {"NZ": (112.0, 12.0)},
                "ASN": {"OD1": (130.0, 20.0)}, "GLN": {"OE1": (130.0, 20.0)}}      # (theta0, sigma_theta) in degrees
ANCHOR_SIGMA_D_METAL, ANCHOR_SIGMA_D_COVALENT = 0.15, 0.10                # A
PP_ANCHOR_PER_ROW = 4


def metal_distance(metal: str, donor_element: str) -> float:
    """Ideal donor-metal distance in A: ``metal_donor_distance`` where it names the pair, else the default of the donor element."""
    key = (str(metal).upper(), str(donor_element).upper())
    if key in metal_donor_distance:
        return metal_donor_distance[key]
    if key[1] not in metal_donor_default:
        raise ValueError(f"no metal-donor distance for donor element {donor_element}")
    return metal_donor_default[key[1]]


def anchor_antecedent(restype: int, slot: int) -> int:
    """The slot the donor in ``slot`` is bonded to, as the angle term reads it: the lowest slot among its covalent neighbours in
    ``bond_rows`` (entries below 1.9 A) -- the neighbour towards the backbone."""
    nb = sorted({int(b) if int(a) == slot else int(a) for rt, a, b, length, _ in bond_rows
                 if int(rt) == restype and length < 1.9 and slot in (int(a), int(b))})
    if not nb:
        raise ValueError(f"{resnames[restype]} slot {slot} has no bonded neighbour")
    return nb[0]


# Explicit hydrogens and the all-atom clashscore (pp_hydrogens / pp_clashscore).  The table is DERIVED from the
# covalent bonds of bond_rows (entries below 1.9 A, as for polar_antecedent) and the atom names; only the hybridisation of the carbons
# and the protonation of the side-chain nitrogens are written out.  Slots of an all-atom row: 0 .. 13 atom14, 14 + k the k-th hydrogen.
PP_AA_SLOTS, PP_H_MAX = 27, 13
H_NONE, H_SUM, H_T2, H_NERF = 0, 1, 2, 3      # how pp_hydrogens places a hydrogen (kind & 15); H_DROP_LINKED: not on a row in `link`
H_DROP_LINKED = 16
H_PREV_C = 14                                 # neighbour code: the C of the previous row (the backbone N's second neighbour)
H_POLAR, H_ROTATABLE, H_AROMATIC = 1, 2, 4    # hydrogen_flags bits
AA_POLAR_H, AA_ACCEPTOR, AA_HYDROGEN, AA_BACKBONE = 1, 2, 4, 8   # allatom_class bits
hydrogen_bond_length = {"C": 1.09, "N": 1.01, "O": 0.96, "S": 1.34}      # nuclear positions, A
sp2_carbons = {"ARG": ("CZ",), "ASN": ("CG",), "ASP": ("CG",), "GLN": ("CD",), "GLU": ("CD",), "HIS": ("CG", "CD2", "CE1"),
               "PHE": ("CG", "CD1", "CD2", "CE1", "CE2", "CZ"), "TYR": ("CG", "CD1", "CD2", "CE1", "CE2", "CZ"),
               "TRP": ("CG", "CD1", "CD2", "CE2", "CE3", "CZ2", "CZ3", "CH2")}
# side-chain nitrogens: (class, hydrogens); HIS is neutral with the hydrogen on NE2, ND1 is bare
nitrogen_hydrogens = {"ARG": {"NE": ("P1", 1), "NH1": ("P2", 2), "NH2": ("P2", 2)}, "ASN": {"ND2": ("P2", 2)}, "GLN": {"NE2": ("P2", 2)},
                      "HIS": {"NE2": ("P1", 1)}, "TRP": {"NE1": ("P1", 1)}, "LYS": {"NZ": ("T3", 3)}}
# the explicit-hydrogen radii as we recall Probe's set; its source is not at hand, so absolute scores belong to THIS table
allatom_radius = {"C": 1.75, "C_carbonyl": 1.65, "N": 1.55, "O": 1.40, "S": 1.80, "H": 1.17, "H_aromatic": 1.00, "H_polar": 1.00}
carbonyl_carbons = {"ASP": ("CG",), "GLU": ("CD",), "ASN": ("CG",), "GLN": ("CD",)}      # next to the backbone C of every residue
T2_ALPHA_DEG, TETRAHEDRAL_DEG = 54.75, 109.5


def _bonded(t):
    """The heavy-atom neighbours of every atom14 slot of residue type t, ascending: bond_rows entries below 1.9 A."""
    nb = [set() for _ in range(14)]
    for rt, a, b, length, _ in bond_rows:
        if int(rt) == t and length < 1.9:
            nb[int(a)].add(int(b))
            nb[int(b)].add(int(a))
    return [sorted(s) for s in nb]


def _hydrogen_tables():
    f32 = np.float32
    cs = lambda deg: (f32(np.cos(np.deg2rad(deg))), f32(np.sin(np.deg2rad(deg))))     # rounded to float once, here
    names = [[] for _ in range(21)]
    parent = -np.ones((21, PP_H_MAX), np.int8)
    place = np.zeros((21, PP_H_MAX, 5), np.int8)
    place[:, :, 1:] = -1
    par = np.zeros((21, PP_H_MAX, 5), np.float32)
    flags = np.zeros((21, PP_H_MAX), np.uint8)
    for t in range(20):
        rn, an, nb = resnames[t], atom14_names[t], _bonded(t)
        k = 0
        for p, nm in enumerate(an):
            if not nm or nm in ("C", "O"):
                continue
            el, stem, heavy = nm[0], "H" + nm[1:], nb[p]
            aromatic = False
            if nm == "N":
                cls, n_h = ("P1bb", 1) if rn != "PRO" else (None, 0)
            elif el == "C":
                aromatic = nm in sp2_carbons.get(rn, ())
                if aromatic:
                    cls, n_h = ("P1", 1) if len(heavy) == 2 else (None, 0)
                else:
                    cls, n_h = {3: ("T1", 1), 2: ("T2", 2), 1: ("T3", 3)}[len(heavy)]
            elif el == "N":
                cls, n_h = nitrogen_hydrogens.get(rn, {}).get(nm, (None, 0))
            else:
                cls, n_h = ("R1", 1) if (rn, nm) in (("SER", "OG"), ("THR", "OG1"), ("TYR", "OH"), ("CYS", "SG")) else (None, 0)
            if not n_h:
                continue
            L = hydrogen_bond_length[el]
            suffix = {1: ("",), 2: ("1", "2") if cls == "P2" else ("2", "3"), 3: ("1", "2", "3")}[n_h]
            for q in range(n_h):
                names[t].append(stem + suffix[q])
                parent[t, k] = p
                flags[t, k] = ((H_POLAR if el in "NOS" else 0) | (H_ROTATABLE if cls == "R1" or (rn, nm) == ("LYS", "NZ") else 0)
                               | (H_AROMATIC if aromatic else 0))
                if cls in ("T1", "P1", "P1bb"):
                    n = heavy + ([H_PREV_C] if cls == "P1bb" else [])
                    place[t, k] = [H_SUM, p] + n + [-1] * (3 - len(n))
                    par[t, k, 0] = L
                elif cls == "T2":
                    c, s = cs(T2_ALPHA_DEG)
                    place[t, k] = [H_T2, p, heavy[0], heavy[1], -1]
                    par[t, k, :3] = [L, c, s if q == 0 else -s]
                else:
                    a = heavy[0]
                    b = [x for x in nb[a] if x != p][0]
                    theta = 120.0 if cls == "P2" else TETRAHEDRAL_DEG
                    phi = {"T3": (60.0, 180.0, 300.0), "P2": (0.0, 180.0), "R1": (180.0,)}[cls][q]
                    place[t, k] = [H_NERF | (H_DROP_LINKED if (rn, nm) == ("CYS", "SG") else 0), p, a, b, -1]
                    par[t, k] = [L, *cs(theta), *cs(phi)]
                k += 1
    return names, parent, place, par, flags


hydrogen_names, hydrogen_parent, hydrogen_place, hydrogen_param, hydrogen_flags = _hydrogen_tables()
# [21] name lists; [21,13] i8 parent slot (-1 = none); [21,13,5] i8 (kind, parent, three neighbour slots or -1; H_NERF: a, b, -1);
# [21,13,5] f32 (L, then cos/sin of alpha with the sign of the side (H_T2) or cos/sin theta, cos/sin phi (H_NERF)); [21,13] u8 flags
hydrogen_count = np.array([len(n) for n in hydrogen_names], np.int32)
allatom_names = [list(atom14_names[t]) + hydrogen_names[t] + [""] * (PP_H_MAX - len(hydrogen_names[t])) for t in range(21)]


def _allatom_tables():
    sep = np.full((21, PP_AA_SLOTS, PP_AA_SLOTS), 9, np.uint8)
    radius = np.zeros((21, PP_AA_SLOTS), np.float32)
    cls = np.zeros((21, PP_AA_SLOTS), np.uint8)
    for t in range(21):
        nb = [list(x) for x in _bonded(t)] + [[] for _ in range(PP_H_MAX)]
        for k in range(int(hydrogen_count[t])):
            p = int(hydrogen_parent[t, k])
            nb[14 + k].append(p)
            nb[p].append(14 + k)
        for s in range(PP_AA_SLOTS):                       # breadth first over the bond graph, hydrogens included
            sep[t, s, s] = 0
            seen, front, d = {s}, [s], 0
            while front and d < 9:
                d += 1
                front = [y for x in front for y in nb[x] if y not in seen and not seen.add(y)]
                for y in front:
                    sep[t, s, y] = min(d, 9)
        rn = resnames[t]
        for s, nm in enumerate(allatom_names[t]):
            if not nm:
                continue
            if s < 14:
                carbonyl = nm == "C" or nm in carbonyl_carbons.get(rn, ())
                radius[t, s] = allatom_radius["C_carbonyl" if carbonyl else nm[0]]
                cls[t, s] = (AA_ACCEPTOR if polar_class[t, s] & POLAR_ACCEPTOR else 0) | (AA_BACKBONE if s < 4 else 0)
            else:
                f, p = int(hydrogen_flags[t, s - 14]), int(hydrogen_parent[t, s - 14])
                radius[t, s] = allatom_radius["H_polar" if f & H_POLAR else "H_aromatic" if f & H_AROMATIC else "H"]
                cls[t, s] = AA_HYDROGEN | (AA_POLAR_H if f & H_POLAR else 0) | (AA_BACKBONE if p < 2 else 0)
    return sep, radius, cls


aa_sep, allatom_default_radius, allatom_class = _allatom_tables()
# [21,27,27] u8 bond-graph separation inside a residue, hydrogens included, clamped at 9 (also: not connected, empty slot);
# [21,27] f32 default radius (0 = empty slot); [21,27] u8 class bits AA_*


# Hydrogen-bond network optimisation (pp_hnet_optimize).  A residue type has at most one MOVER: a rotor (the
# rotatable hydrogens above turn about the bond to their parent) or a flip (the rigid group of one chi turned by pi, hydrogens with
# it).  Only the flipped chi of each flip type and the rotor states are written out; the moved atoms are derived.
MOVER_NONE, MOVER_ROTOR, MOVER_FLIP = 0, 1, 2
PP_HNET_STATES, PP_HNET_ROT_H, PP_HNET_MOVED = 12, 3, 7
mover_flip_chi = {"ASN": 1, "GLN": 2, "HIS": 1}          # index of the flipped chi: chi2, chi3, chi2
# dihedral of the rotor's first hydrogen in state c, degrees; a lysine's HZ2 / HZ3 follow at + 120 / + 240
mover_rotor_states = {"SER": [180.0 + 30.0 * c for c in range(12)], "THR": [180.0 + 30.0 * c for c in range(12)],
                      "CYS": [180.0 + 30.0 * c for c in range(12)], "TYR": [180.0, 0.0], "LYS": [60.0 + 30.0 * c for c in range(4)]}


def _mover_tables():
    f32 = np.float32
    table = np.zeros((21, 4), np.int32)                    # (kind, states, bit mask of the moved slots, 0)
    rot = np.zeros((21, PP_HNET_STATES, PP_HNET_ROT_H, 2), np.float32)
    ext = np.zeros(21, np.float32)
    for t in range(20):
        rn = resnames[t]
        hyd = [k for k in range(int(hydrogen_count[t])) if hydrogen_flags[t, k] & H_ROTATABLE]
        moved = []
        if rn in mover_flip_chi:
            heavy = [s for s in range(14) if atom14_names[t][s] and int(atom14_to_group[t, s]) == 4 + mover_flip_chi[rn]]
            moved = heavy + [14 + k for k in range(int(hydrogen_count[t])) if int(hydrogen_parent[t, k]) in heavy]
            table[t, :2] = MOVER_FLIP, 2
        elif hyd:
            states = mover_rotor_states[rn]
            moved = [14 + k for k in hyd]
            table[t, :2] = MOVER_ROTOR, len(states)
            for c, deg in enumerate(states):
                for j, k in enumerate(hyd):
                    if c == 0:
                        rot[t, 0, j] = hydrogen_param[t, k, 3:5]           # the very values pp_hydrogens uses
                    else:
                        a = np.deg2rad(deg + 120.0 * j)
                        rot[t, c, j] = f32(np.cos(a)), f32(np.sin(a))
        if not moved:
            continue
        assert len(moved) <= PP_HNET_MOVED and len(hyd) <= PP_HNET_ROT_H
        table[t, 2] = sum(1 << s for s in moved)
        # the longest way along the bonds from CA to a moved atom, ideal lengths: no moved atom is ever farther from CA than this
        dist = {1: 0.0}
        edges = [(int(a), int(b), float(length)) for rt, a, b, length, _ in bond_rows if int(rt) == t and length < 1.9]
        edges += [(int(hydrogen_parent[t, k]), 14 + k, hydrogen_bond_length[atom14_names[t][int(hydrogen_parent[t, k])][0]])
                  for k in range(int(hydrogen_count[t]))]
        for _ in range(PP_AA_SLOTS):
            for a, b, length in edges:
                for u, v in ((a, b), (b, a)):
                    if u in dist and dist[u] + length < dist.get(v, 1e9):
                        dist[v] = dist[u] + length
        ext[t] = f32(max(dist[s] for s in moved))
    return table, rot, ext


mover_table, mover_rotor_cs, mover_extent = _mover_tables()
# [21,4] i32 (kind MOVER_*, number of states, bit mask over the 27 all-atom slots of the atoms that move, 0); [21,12,3,2] f32 cos / sin
# of the dihedral of the rotor's j-th hydrogen in state c (state 0: hydrogen_param's); [21] f32 sum of ideal bond lengths from CA to
# the farthest moved atom


def mover_moved_names(t):
    """Names of the moved atoms of residue type t, in slot order."""
    return [allatom_names[t][s] for s in range(PP_AA_SLOTS) if int(mover_table[t, 2]) >> s & 1]


def mover_state_angle(t, state):
    """What ``hnet.csv`` prints as the angle of a mover of type t in `state`: the dihedral of a rotor's first hydrogen in degrees
    (wrapped to [0, 360)), 0 / 180 for a flip."""
    if int(mover_table[t, 0]) == MOVER_ROTOR:
        return float(mover_rotor_states[resnames[t]][int(state)] % 360.0)
    return 180.0 * int(state)


# All-atom chi refinement (pp_chi_refine).  The atoms a chi step can move are the atom14 slots 5 .. 13 and
# every hydrogen whose parent, or one of the atoms it is built from, is such a slot (the hydrogens on CB are built from CG); the
# kernel derives them from ``hydrogen_place``.  Here only how far from CA they can get.


def _refine_extent():
    ext = np.zeros(21, np.float32)
    for t in range(20):
        if not chi_angles_mask[t].any():
            continue
        moved = [s for s in range(5, 14) if atom14_names[t][s]]
        moved += [14 + k for k in range(int(hydrogen_count[t])) if any(5 <= int(v) <= 13 for v in hydrogen_place[t, k, 1:])]
        # as mover_extent: the way along the bonds from CA to the farthest moved atom, ideal lengths -- without proline's N-CD bond,
        # which the reconstruction at arbitrary angles does not close
        dist = {1: 0.0}
        edges = [(int(a), int(b), float(length)) for rt, a, b, length, _ in bond_rows
                 if int(rt) == t and length < 1.9 and not (min(int(a), int(b)) == 0 and max(int(a), int(b)) >= 5)]
        edges += [(int(hydrogen_parent[t, k]), 14 + k, hydrogen_bond_length[atom14_names[t][int(hydrogen_parent[t, k])][0]])
                  for k in range(int(hydrogen_count[t]))]
        for _ in range(PP_AA_SLOTS):
            for a, b, length in edges:
                for u, v in ((a, b), (b, a)):
                    if u in dist and dist[u] + length < dist.get(v, 1e9):
                        dist[v] = dist[u] + length
        ext[t] = np.float32(max(dist[s] for s in moved))
    return ext


refine_extent = _refine_extent()
# [21] f32 sum of ideal bond lengths from CA to the farthest atom a chi step can move (0: the type has no chi)


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
