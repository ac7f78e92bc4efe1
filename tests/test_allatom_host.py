"""CPU: the hydrogen table, the oracle and the texts of the all-atom clashscore.

The table of ``packppi_amd.constants`` is derived from the bond list; here it is held against literal lists (this file's names, the
oracle's chemistry in tests/allatom_oracle.py) and against chemistry's valences.  The oracle itself is held against the definition:
bond lengths, angles, dihedrals, chirality, and float32 against float64."""
import functools

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc

from . import allatom_oracle as A
from . import polar_oracle as O

COUNTS = {3: "GLY", 4: "ASP", 5: "ALA SER CYS", 6: "GLU ASN", 7: "THR PRO HIS", 8: "GLN", 9: "VAL MET PHE TYR", 10: "TRP", 11: "LEU ILE",
          13: "LYS ARG"}
# PDB v3 names, parents in atom14 slot order
NAMES = {
    "ALA": "H HA HB1 HB2 HB3", "ARG": "H HA HB2 HB3 HG2 HG3 HD2 HD3 HE HH11 HH12 HH21 HH22", "ASN": "H HA HB2 HB3 HD21 HD22",
    "ASP": "H HA HB2 HB3", "CYS": "H HA HB2 HB3 HG", "GLN": "H HA HB2 HB3 HG2 HG3 HE21 HE22", "GLU": "H HA HB2 HB3 HG2 HG3",
    "GLY": "H HA2 HA3", "HIS": "H HA HB2 HB3 HD2 HE1 HE2", "ILE": "H HA HB HG12 HG13 HG21 HG22 HG23 HD11 HD12 HD13",
    "LEU": "H HA HB2 HB3 HG HD11 HD12 HD13 HD21 HD22 HD23", "LYS": "H HA HB2 HB3 HG2 HG3 HD2 HD3 HE2 HE3 HZ1 HZ2 HZ3",
    "MET": "H HA HB2 HB3 HG2 HG3 HE1 HE2 HE3", "PHE": "H HA HB2 HB3 HD1 HD2 HE1 HE2 HZ", "PRO": "HA HB2 HB3 HG2 HG3 HD2 HD3",
    "SER": "H HA HB2 HB3 HG", "THR": "H HA HB HG1 HG21 HG22 HG23", "TRP": "H HA HB2 HB3 HD1 HE1 HE3 HZ2 HZ3 HH2",
    "TYR": "H HA HB2 HB3 HD1 HD2 HE1 HE2 HH", "VAL": "H HA HB HG11 HG12 HG13 HG21 HG22 HG23", "UNK": "",
}
FIXTURES = ("c24", "c64", "three_chains", "damaged64", "1BRS", "2FTL")


def test_counts_per_residue_type():
    assert rc.PP_AA_SLOTS == 27 and rc.PP_H_MAX == 13
    want = {name: n for n, names in COUNTS.items() for name in names.split()}
    want["UNK"] = 0
    assert {rc.resnames[t]: int(rc.hydrogen_count[t]) for t in range(21)} == want
    assert int(rc.hydrogen_count.sum()) == 157 and int((rc.hydrogen_parent >= 0).sum()) == 157


def test_names_against_the_literal_lists():
    for t, rn in enumerate(rc.resnames):
        assert rc.hydrogen_names[t] == NAMES[rn].split(), rn
        assert rc.allatom_names[t][:14] == list(rc.atom14_names[t]) and rc.allatom_names[t][14:14 + len(rc.hydrogen_names[t])] == NAMES[rn].split()
        assert len(rc.allatom_names[t]) == 27
        k = int(rc.hydrogen_count[t])
        assert (rc.hydrogen_place[t, k:, 0] == 0).all() and (rc.hydrogen_place[t, :k, 0] != 0).all()
        par = rc.hydrogen_parent[t, :k]
        assert (np.diff(par) >= 0).all(), "parents in slot order, each parent's hydrogens consecutive"


def test_valences():
    """Heavy neighbours + hydrogens: 4 on sp3 carbon and NZ, 3 on sp2 carbon and on amide / guanidinium / ring / backbone N, 2 on
    the O and S that carry one."""
    seen = 0
    for t, rn in enumerate(rc.resnames[:20]):
        nb = rc._bonded(t)
        for s, nm in enumerate(rc.atom14_names[t]):
            if not nm:
                continue
            n_h = int((rc.hydrogen_parent[t] == s).sum())
            heavy = len(nb[s]) + (1 if nm == "N" else 0) + (1 if nm == "C" else 0)          # the peptide bonds to the neighbours
            total = heavy + n_h
            if nm[0] == "C":
                sp2 = nm == "C" or nm in rc.sp2_carbons.get(rn, ())
                assert total == (3 if sp2 else 4), (rn, nm, total)
            elif nm[0] == "N" and n_h:
                assert total == (4 if (rn, nm) == ("LYS", "NZ") else 3), (rn, nm, total)
            elif nm[0] in "OS" and n_h:
                assert total == 2, (rn, nm, total)
            elif nm == "N":
                assert rn == "PRO" and total == 3
            seen += n_h
    assert seen == 157
    t = rc.resname_to_idx["HIS"]
    assert "HD1" not in rc.hydrogen_names[t] and "HE2" in rc.hydrogen_names[t]            # neutral, the hydrogen on NE2


def test_flags_and_classes():
    rot = {(rc.resnames[t], rc.hydrogen_names[t][k]) for t in range(20) for k in range(int(rc.hydrogen_count[t]))
           if rc.hydrogen_flags[t, k] & rc.H_ROTATABLE}
    assert rot == A.ROTATABLE
    tb = A.get_tables()
    for t in range(21):
        assert tb["names"][t] == rc.allatom_names[t]
    assert np.array_equal(tb["radius"], rc.allatom_default_radius) and np.array_equal(tb["acls"], rc.allatom_class)
    drop = [(t, k) for t in range(21) for k in range(13) if rc.hydrogen_place[t, k, 0] & rc.H_DROP_LINKED]
    assert drop == [(rc.resname_to_idx["CYS"], 4)]
    phe = rc.resname_to_idx["PHE"]
    assert all(rc.hydrogen_flags[phe, k] & rc.H_AROMATIC for k in range(4, 9)) and not rc.hydrogen_flags[phe, 2] & rc.H_AROMATIC


def test_aa_sep():
    s = rc.aa_sep
    assert s.shape == (21, 27, 27) and s.dtype == np.uint8 and s.max() == 9
    assert np.array_equal(s, s.transpose(0, 2, 1)) and (s[:, np.arange(27), np.arange(27)] == 0).all()
    assert np.array_equal(s, A.get_tables()["sep"])
    ala = rc.resname_to_idx["ALA"]
    assert s[ala, 0, 1] == 1 and s[ala, 14, 0] == 1 and s[ala, 14, 15] == 3 and s[ala, 16, 17] == 2 and s[ala, 3, 16] == 4
    lys = rc.resname_to_idx["LYS"]
    assert s[lys, 0, 8] == 6 and s[lys, 14, 26] == 8 and s[ala, 0, 5] == 9               # an empty slot is as far as the clamp


# ---- the oracle against the definition ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def placed(name, dtype=np.float64):
    b = O.batch(name)
    X, _, _, chain, offs = O.arrays(b)
    am, rt = b["atom_mask"].reshape(-1, 14).numpy(), b["residue_type"].reshape(-1).numpy()
    h, m, lp = A.hydrogens(X.astype(dtype), am, rt, chain, offs, dtype=dtype)
    return X.astype(np.float64), am, rt, chain, offs, h, m, lp


def _angle(a, b, c):
    u, v = a - b, c - b
    return np.degrees(np.arccos(np.clip(np.dot(u, v) / np.linalg.norm(u) / np.linalg.norm(v), -1, 1)))


def _dihedral(p0, p1, p2, p3):
    b0, b1, b2 = p0 - p1, p2 - p1, p3 - p2
    b1 = b1 / np.linalg.norm(b1)
    v, w = b0 - np.dot(b0, b1) * b1, b2 - np.dot(b2, b1) * b1
    return np.degrees(np.arctan2(np.dot(np.cross(b1, v), w), np.dot(v, w))) % 360.0


@pytest.mark.parametrize("name", FIXTURES)
def test_geometric_invariants(name):
    X, am, rt, chain, offs, h, m, lp = placed(name)
    tb = A.get_tables()
    n_h = n_nerf = n_ha = 0
    for n in range(len(rt)):
        hyd = tb["hyd"][int(rt[n])]
        for k, (cls, p, at, q, L) in enumerate(hyd):
            if not m[n, k]:
                continue
            n_h += 1
            P, H = X[n, p], h[n, k]
            assert abs(np.linalg.norm(H - P) - L) <= 1e-6
            pos = lambda s: X[n - 1, 2] if s == -2 else X[n, s]
            if cls == "T1":
                for a in at:                                             # away from three neighbours: tetrahedral within 2 degrees on
                    ang = _angle(H, P, pos(a))                           # ideal parents; real ones are checked for the side only
                    assert ang > 90.0
            elif cls in ("T3", "R1", "P2"):
                theta, phis = A.ANGLES[cls]
                assert abs(_angle(H, P, pos(at[0])) - theta) <= 2.0
                d = _dihedral(H, P, pos(at[0]), pos(at[1]))
                assert min(abs(d - phis[q]), 360.0 - abs(d - phis[q])) <= 1e-3, (cls, d, phis[q])
                n_nerf += 1
            elif cls == "T2":
                assert abs(_angle(H, P, h[n, k + (1 if q == 0 else -1)]) - 109.5) <= 2.0 if m[n, k + (1 if q == 0 else -1)] else True
            elif cls in ("P1", "P1bb"):
                a1, a2 = _angle(H, P, pos(at[0])), _angle(H, P, pos(at[1]))
                assert abs(a1 - a2) <= 1e-3 and a1 > 90.0              # on the bisector, in the plane, pointing away
                nrm = np.cross(pos(at[0]) - P, pos(at[1]) - P)
                assert abs(np.dot(H - P, nrm / np.linalg.norm(nrm))) <= 1e-6
        # no two hydrogens of one parent closer than 1.5 A
        for k1 in range(len(hyd)):
            for k2 in range(k1 + 1, len(hyd)):
                if hyd[k1][1] == hyd[k2][1] and m[n, k1] and m[n, k2]:
                    assert np.linalg.norm(h[n, k1] - h[n, k2]) >= 1.5
        # HA of an L residue: on the other side of the N-CA-C plane from CB, and CB on the L side
        names = tb["names"][int(rt[n])]
        if "HA" in names and m[n, names.index("HA") - 14] and am[n, 4]:
            nrm = np.cross(X[n, 0] - X[n, 1], X[n, 2] - X[n, 1])
            cb, ha = np.dot(X[n, 4] - X[n, 1], nrm), np.dot(h[n, names.index("HA") - 14] - X[n, 1], nrm)
            assert cb > 0 > ha, "a D residue would have CB and HA the other way round"
            n_ha += 1
    assert n_h == int(m.sum()) >= 150 and n_nerf >= 20 and n_ha >= 15


def test_ideal_parents_give_ideal_angles():
    """On the ideal geometry of ``atom14`` (a synthetic complex) every H-parent-neighbour angle of a T1 / T2 hydrogen is within
    2 degrees of 109.5, except on CA and in proline's ring, whose angles the backbone sets."""
    X, am, rt, chain, offs, h, m, lp = placed("c64")
    tb = A.get_tables()
    n = 0
    for r in range(len(rt)):
        if int(rt[r]) == 14:
            continue
        for k, (cls, p, at, q, L) in enumerate(tb["hyd"][int(rt[r])]):
            if cls in ("T1", "T2") and p >= 4 and m[r, k]:
                for a in at:
                    assert abs(_angle(h[r, k], X[r, p], X[r, a]) - 109.5) <= 2.0, (rc.resnames[int(rt[r])], k)
                    n += 1
    assert n >= 100


def test_link_prev_and_missing_atoms():
    X, am, rt, chain, offs, h, m, lp = placed("damaged64")
    full = A.hydrogens(X, np.ones_like(am), rt, chain, offs)[1]
    assert (m <= full).all() and m.sum() < full.sum()
    tb = A.get_tables()
    for n in range(len(rt)):
        for k, (cls, p, at, q, L) in enumerate(tb["hyd"][int(rt[n])]):
            needs = [p] + [a for a in at if a >= 0]
            if any(am[n, a] == 0 for a in needs):
                assert m[n, k] == 0
    assert lp[0] == 0 and lp[32] == 0 and lp[1:32].sum() >= 25                              # the first row of a chain has no H
    assert (m[lp == 0][:, 0][rt[lp == 0] != 14] == 0).all()


# ---- float32 against float64 ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def clashes(name, dtype):
    b = O.batch(name)
    X, _, _, chain, offs = O.arrays(b)
    am, rt = b["atom_mask"].reshape(-1, 14).numpy(), b["residue_type"].reshape(-1).numpy()
    h, m, lp = A.hydrogens(X.astype(dtype), am, rt, chain, offs, dtype=dtype)
    return A.clash(X.astype(dtype), h, m, A.default_radius(rt, am), rt, chain, offs, lp, dtype=dtype)


@pytest.mark.parametrize("name", ("c24", "1BRS", "2FTL"))
def test_float32_and_float64_agree_outside_the_ambiguous_pairs(name):
    a, b = clashes(name, np.float32), clashes(name, np.float64)
    amb = {p[:4] for p in b["near"] if abs(p[4]) <= 1e-4}
    differ = set(a["pairs"]) ^ set(b["pairs"])
    print(f"{name}: {len(b['pairs'])} overlaps, {len(differ)} differ, {len(amb)} ambiguous of {len(b['near'])} within 0.5 A")
    assert len(b["near"]) >= 500 and len(amb) <= 1e-3 * len(b["near"])
    assert differ <= amb
    if not amb:
        for k in ("n_clash", "partners", "res", "seg"):
            assert a[k].tobytes() == b[k].tobytes()


def test_recorded_figures_of_1brs_keep_their_order():
    """crystal < side chains rebuilt from their own angles < uniform random angles < all angles 0 (DESIGN.md section 29 records the
    figures; only the order is asserted, it holds by factors)."""
    from oracle import ref_cpu
    b = O.batch("1BRS")
    X, _, _, chain, offs = O.arrays(b)
    am, rt = b["atom_mask"].reshape(-1, 14).numpy(), b["residue_type"].reshape(-1).numpy()
    g = torch.Generator().manual_seed(0)
    sets = [None, b["SC_D"], ((torch.rand(b["SC_D"].shape, generator=g) * 2 - 1) * np.pi) * b["SC_D_mask"], torch.zeros_like(b["SC_D"])]
    scores = []
    for chi in sets:
        x = X if chi is None else ref_cpu.atom14_coords(b["X"], b["residue_type"], b["BB_D"], chi).reshape(-1, 14, 3).numpy().astype(np.float32)
        x = np.where(am[..., None] != 0, x, X)
        h, m, lp = A.hydrogens(x, am, rt, chain, offs, dtype=np.float32)
        seg = A.clash(x, h, m, A.default_radius(rt, am), rt, chain, offs, lp)["seg"]
        scores.append(float(A.clashscore(seg)[0]))
        assert seg[0, 0] == 2998
    print("1BRS clashscore: crystal %.1f, rebuilt %.1f, random %.1f, zero %.1f" % tuple(scores))
    assert scores[0] < scores[1] < scores[2] < scores[3]


# ---- texts ---------------------------------------------------------------------------------------------------------------------------------
def test_structure_h_pdb_round_trip(tmp_path):
    from packppi_amd.pdb_io import from_pdb_file, to_pdb, to_pdb_hydrogens
    p = O.protein("1BRS")
    X, am, rt, chain, offs, h, m, lp = placed("1BRS")
    text, plain = to_pdb_hydrogens(p, h, m), to_pdb(p)
    lines = text.split("\n")
    hyd = [ln for ln in lines if ln.startswith("ATOM") and ln[76:78].strip() == "H"]
    assert len(hyd) == int(m.sum()) and all(len(ln) == 80 for ln in lines[:-1])
    strip = lambda ln: ln[:6] + ln[11:]                                  # the serial numbers are renumbered
    heavy = [ln for ln in lines if ln not in set(hyd)]
    assert [strip(ln) for ln in heavy] == [strip(ln) for ln in plain.split("\n")]
    serials = [int(ln[6:11]) for ln in lines if ln.startswith(("ATOM", "TER"))]
    assert serials == list(range(1, len(serials) + 1))
    first = [ln[12:16].strip() for ln in lines[1:17]]
    assert first[:7] == ["N", "CA", "C", "O", "CB", "CG1", "CG2"] and first[7:14] == ["HA", "HB", "HG11", "HG12", "HG13", "HG21", "HG22"]
    assert any(ln[12:16] == "HH11" for ln in hyd) and any(ln[12:16] == " HA " for ln in hyd)
    (tmp_path / "h.pdb").write_text(text)
    (tmp_path / "plain.pdb").write_text(plain)
    a, b = from_pdb_file(tmp_path / "h.pdb"), from_pdb_file(tmp_path / "plain.pdb")
    for k in b:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def test_clashes_csv_text():
    from packppi_amd.analysis import CLASHES_CSV_HEADER, clash_pairs, clashes_csv_text
    p = O.protein("1BRS")
    X, am, rt, chain, offs, h, m, lp = placed("1BRS")
    ref = clashes("1BRS", np.float64)
    radius = A.default_radius(rt, am)
    assert clash_pairs(ref["partners"]) == [((i, x), (j, y)) for i, x, j, y in sorted(ref["pairs"], key=lambda q: (q[0] * 27 + q[1], q[2] * 27 + q[3]))]
    text = clashes_csv_text(p, X, h, ref["partners"], radius)
    rows = [ln.split(",") for ln in text.splitlines()]
    assert rows[0] == CLASHES_CSV_HEADER.split(",") and len(rows) == 1 + len(ref["pairs"]) and text.endswith("\n")
    assert all(float(r[9]) >= 0.4 - 5e-4 and r[10] == "" for r in rows[1:])                # a serious overlap is at least the cut
    assert any(r[3].startswith("H") or r[7].startswith("H") for r in rows[1:])
    # against itself everything is kept; against nothing everything is gained
    kept = clashes_csv_text(p, X, h, ref["partners"], radius, native_partners=ref["partners"])
    assert {ln.rsplit(",", 1)[1] for ln in kept.splitlines()[1:]} == {"kept"}
    none = -np.ones_like(ref["partners"])
    gained = clashes_csv_text(p, X, h, ref["partners"], radius, native_partners=none)
    lost = clashes_csv_text(p, X, h, none, radius, native_partners=ref["partners"])
    assert {ln.rsplit(",", 1)[1] for ln in gained.splitlines()[1:]} == {"gained"}
    assert {ln.rsplit(",", 1)[1] for ln in lost.splitlines()[1:]} == {"lost"} and lost.count("\n") == kept.count("\n")


def test_the_command_lines_take_the_flags_only_when_given():
    from packppi_amd.cli import eval_diffusion, mutate, proximal_optimize
    base = ["--input", "x.pdb", "--outdir", "o", "--molprobity_clash_loc", "none"]
    for tool in (eval_diffusion, proximal_optimize):
        plain = tool.parse_args(base)
        assert not hasattr(plain, "clashscore") and not hasattr(plain, "hydrogens")
        both = tool.parse_args(base + ["--clashscore", "--hydrogens"])
        assert both.clashscore is True and both.hydrogens is True
    ns = mutate.build_parser().parse_args(["--input", "x.pdb", "--outdir", "o", "--mutstr", "LA87F", "--seed", "1", "--hydrogens"])
    assert ns.hydrogens is True and not hasattr(ns, "clashscore")


def test_protein_analysis_keeps_its_default(tmp_path):
    from packppi_amd.analysis import ProteinAnalysis
    assert ProteinAnalysis("none", str(tmp_path)).device_clashscore is False
    assert ProteinAnalysis("none", str(tmp_path), "cuda", True).device_clashscore is True
