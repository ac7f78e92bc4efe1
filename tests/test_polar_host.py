"""Polar contacts on the host (pp_polar): the class and antecedent tables, the NumPy restatement in both
precisions on the synthetic complexes and the two fixtures, symmetry, the CSV texts, ``polar_recovery`` and the argument rules.

Figures the restatement gives (bonds, between chains, with a side-chain atom, salt bridges (between chains)): 1BRS 241 / 13 / 91 /
12 (3), make_complex(24, 5) 14 / 3 / 5 / 3 (2), (64, 11) 44 / 10 / 16 / 4 (1), (97, 267) 72 / 10 / 29 / 4 (3),
(45, 3, n_chains=3) 23 / 3 / 8 / 3 (1).  2FTL gives 286 bonds under the row rule of step 6 (287 with residue numbers: one
backbone pair at a numbering gap that is no row gap)."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc

from . import polar_oracle as O

GOLD = O.GOLD


protein, batch, reference, SINGLES = O.protein, O.batch, O.reference, O.SINGLES
FIGURES = {"1BRS": (241, 13, 91, 12, 3), "c24": (14, 3, 5, 3, 2), "c64": (44, 10, 16, 4, 1), "c97": (72, 10, 29, 4, 3),
           "three_chains": (23, 3, 8, 3, 1)}


# ---- the tables ------------------------------------------------------------------------------------------------------------------------------
def test_tables_are_the_oracles_lists():
    cls, ante = O.tables()
    assert rc.polar_class.dtype == np.uint8 and rc.polar_class.shape == (21, 14)
    assert rc.polar_antecedent.dtype == np.int8 and rc.polar_antecedent.shape == (21, 14, 2)
    assert np.array_equal(rc.polar_class, cls) and np.array_equal(rc.polar_antecedent, ante)
    assert (rc.polar_class[20] == 0).all()                       # the unknown residue has no polar atom


def test_every_polar_slot_has_bonded_antecedents():
    bonded = {}
    for t, a, b, length, _ in rc.bond_rows:
        if length < 1.9:
            bonded.setdefault(int(t), set()).update({(int(a), int(b)), (int(b), int(a))})
    n = 0
    for t in range(20):
        for s in range(14):
            an = [int(a) for a in rc.polar_antecedent[t, s] if a >= 0]
            if rc.polar_class[t, s] == 0:
                assert not an
                continue
            n += 1
            assert rc.atom14_names[t][s] and 1 <= len(an) <= 2 and len(set(an)) == len(an)
            for a in an:
                assert (s, a) in bonded[t], (rc.resnames[t], rc.atom14_names[t][s], rc.atom14_names[t][a])
            # and none is left out: the antecedents are ALL heavy atoms bonded to the atom
            assert sorted(an) == sorted(b for a, b in bonded[t] if a == s)
    assert n == 20 + 19 + 18        # 20 O, 19 N (no PRO), 18 side-chain atoms (ARG 3, ASN ASP GLN GLU HIS 2 each, LYS SER THR TRP TYR 1)


def test_atoms_that_are_not_polar():
    def c(res, atom):
        t = rc.resname_to_idx[res]
        return int(rc.polar_class[t, rc.atom14_names[t].index(atom)])
    assert c("PRO", "N") == 0 and c("MET", "SD") == 0 and c("CYS", "SG") == 0 and c("ALA", "CA") == 0 and c("TRP", "CZ2") == 0
    assert c("ALA", "N") == 1 and c("PRO", "O") == 2 and c("SER", "OG") == 3 and c("HIS", "ND1") == 3
    assert c("LYS", "NZ") == 5 and c("ARG", "NH2") == 5 and c("ASP", "OD2") == 10 and c("GLU", "OE1") == 10
    assert c("ASN", "ND2") == 1 and c("ASN", "OD1") == 2 and c("TRP", "NE1") == 1
    t = rc.resname_to_idx["HIS"]
    names = rc.atom14_names[t]
    assert sorted(names[a] for a in rc.polar_antecedent[t, names.index("ND1")]) == ["CE1", "CG"]
    t = rc.resname_to_idx["ARG"]
    names = rc.atom14_names[t]
    assert sorted(names[a] for a in rc.polar_antecedent[t, names.index("NE")]) == ["CD", "CZ"]


def test_a_missing_antecedent_takes_the_class_away():
    b = batch("damaged64")
    cls, ante = O.classify(b["residue_type"], b["atom_mask"])
    full, _ = O.classify(b["residue_type"], np.ones_like(np.asarray(b["atom_mask"])))
    am = np.asarray(b["atom_mask"]).reshape(-1, 14) != 0
    gone = (full != 0) & (cls == 0)
    assert ((cls != 0) <= am).all()
    # six polar atoms are missing themselves; one is there, but its antecedent is not
    assert int((gone & ~am).sum()) == 6 and int((gone & am).sum()) == 1


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIGURES))
def test_the_figures_of_the_restatement(name):
    seg = reference(name)["seg"][0]
    assert (seg[0], seg[1], seg[2], seg[4], seg[5]) == FIGURES[name]


@pytest.mark.parametrize("name", SINGLES + ("c40", "c36"))
def test_fp32_agrees_with_fp64_outside_ambiguous_pairs(name):
    X, cls, ante, chain, offs = O.arrays(batch(name))
    bad, amb, cand = O.compare_precisions(X, cls, ante, chain, offs)
    print(f"{name}: {cand} candidate pairs within 4.0 A, {amb} ambiguous, {bad} differ outside them")
    assert cand > 50 and bad == 0
    assert amb <= 1e-3 * cand
    if name not in ("c40", "c36"):
        assert amb == 0


@pytest.mark.parametrize("name", SINGLES)
def test_the_relation_is_symmetric_and_the_sums_add_up(name):
    r = reference(name)
    g = r["segments"][0]
    assert np.array_equal(g["hb"], g["hb"].T) and np.array_equal(g["salt"], g["salt"].T) and not g["hb"].diagonal().any()
    p, n = r["partners"], r["n_partners"]
    listed = set()
    for row, s, k in zip(*np.nonzero(p >= 0)):
        listed.add((int(row) * 14 + int(s), int(p[row, s, k])))
    assert n[..., 0].max() <= O.CAP                                      # no list of these cases is cut: the lists are complete
    assert all((b, a) in listed for a, b in listed)
    assert len(listed) == 2 * r["seg"][0, 0] == n[..., 0].sum() == r["res"][:, :4].sum()
    assert r["res"][:, 1].sum() + r["res"][:, 3].sum() == 2 * r["seg"][0, 1]
    assert r["res"][:, 4].sum() == 2 * (r["seg"][0, 4] - r["seg"][0, 5]) and r["res"][:, 5].sum() == 2 * r["seg"][0, 5]
    assert r["seg"][0, 7] == r["res"][:, 7].sum() and (np.diff(np.where(p >= 0, p, 1 << 30), axis=-1) >= 0).all()
    assert r["seg"][0, 3] >= 1 and r["seg"][0, 4] >= 1                   # not vacuous


def test_nan_positions_bond_nothing():
    X, cls, ante, chain, offs = O.arrays(batch("c24"))
    X = X.copy()
    r0 = O.contacts(X, cls, ante, chain, offs)
    row = int(np.nonzero(r0["res"][:, :4].sum(1))[0][0])
    X[row] = np.nan
    r1 = O.contacts(X, cls, ante, chain, offs)
    assert (r1["n_partners"][row] == 0).all() and (r1["partners"][row] == -1).all()
    assert r1["res"][row, 7] == (cls[row] != 0).sum() and r1["seg"][0, 0] < r0["seg"][0, 0]


# ---- the texts -------------------------------------------------------------------------------------------------------------------------------
def test_polar_csv_format():
    from packppi_amd.analysis import POLAR_CSV_HEADER, polar_csv_text
    prot = dict(chain_id=np.array(["A", "A", "B"]), residue_index=np.array([7, 8, -2]), aaindex=np.array([rc.resname_to_idx[n] for n in ("ALA", "SER", "GLN")]))
    res = np.arange(16).reshape(2, 8)
    text = polar_csv_text(prot, res)
    assert text.splitlines() == [POLAR_CSV_HEADER, "A,7,ALA,0,1,2,3,4,5,6,7", "A,8,SER,8,9,10,11,12,13,14,15", "B,-2,GLN,0,0,0,0,0,0,0,0"]
    assert text.endswith("\n")
    buns = np.zeros((2, 14), bool)
    buns[1, [3, 5]] = True
    lines = polar_csv_text(prot, res, buns).splitlines()
    assert lines[0] == POLAR_CSV_HEADER + ",buns" and [ln.rsplit(",", 1)[1] for ln in lines[1:]] == ["0", "2", "0"]


def test_hbonds_csv_format_and_status():
    from packppi_amd.analysis import HBONDS_CSV_HEADER, hbonds_csv_text, polar_bonds
    prot = dict(chain_id=np.array(["A", "A", "B"]), residue_index=np.array([7, 8, 3]), aaindex=np.array([rc.resname_to_idx[n] for n in ("ALA", "SER", "GLN")]))
    og, oe1 = rc.atom14_names[rc.resname_to_idx["SER"]].index("OG"), rc.atom14_names[rc.resname_to_idx["GLN"]].index("OE1")
    xyz = np.zeros((3, 14, 3))
    xyz[1, og] = (3.0, 0, 0)
    xyz[2, oe1] = (0, 0, 2.5)
    here = -np.ones((3, 14, 4), np.int64)
    here[0, 3, 0] = 1 * 14 + og             # A7 O -- A8 OG, listed from one side only
    here[0, 0, 0] = 2 * 14 + 3              # A7 N -- B3 O, backbone but between chains
    here[2, 3, 0] = 0
    here[0, 0, 1] = 1 * 14 + 3              # A7 N -- A8 O: backbone within a chain, not written
    assert polar_bonds(here) == [((0, 0), (1, 3)), ((0, 0), (2, 3)), ((0, 3), (1, og))]
    lines = hbonds_csv_text(prot, xyz, here).splitlines()
    assert lines == [HBONDS_CSV_HEADER, "A,7,ALA,N,B,3,GLN,O,0.000,", "A,7,ALA,O,A,8,SER,OG,3.000,"]
    native = -np.ones((3, 14, 4), np.int64)
    native[1, og, 0] = 3                     # the same A7 O -- A8 OG, from the other side
    native[2, oe1, 0] = 0                     # B3 OE1 -- A7 N: lost
    lines = hbonds_csv_text(prot, xyz, here, native).splitlines()
    assert lines[1:] == ["A,7,ALA,N,B,3,GLN,O,0.000,gained", "A,7,ALA,N,B,3,GLN,OE1,2.500,lost", "A,7,ALA,O,A,8,SER,OG,3.000,kept"]


def test_obstacle_polar_marks_nitrogen_and_oxygen():
    from packppi_amd.analysis import obstacle_polar
    assert obstacle_polar(None) is None
    got = obstacle_polar(dict(element=["C", "N", "O", "P", "S", "n", "CL"]))
    assert got.dtype == np.uint8 and got.tolist() == [0, 1, 1, 0, 0, 1, 0]


def test_obstacle_polar_rides_with_the_batch():
    from packppi_amd.batch import pack, replicate, split
    from packppi_amd.featurize import protein_to_batch
    xyz = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 9]], np.float32)
    ob = dict(xyz=xyz, radius=np.full(3, 1.5, np.float32), element=["N", "C", "O"])
    b = protein_to_batch(protein("c24"), obstacles=ob)
    assert b["obstacle_polar"].dtype == torch.uint8 and b["obstacle_polar"].tolist() == [1, 0, 1]
    assert split(b)[0]["obstacle_polar"].tolist() == [1, 0, 1]
    plain = protein_to_batch(protein("c24"), obstacles=dict(xyz=xyz[:2], radius=np.ones(2, np.float32)))      # no elements: no key
    assert "obstacle_polar" not in plain and "obstacle_xyzr" in plain
    assert "obstacle_polar" not in pack([plain, batch("c36")]) and "obstacle_polar" not in batch("c24")
    p = pack([b, batch("c36"), plain])
    assert p["obstacle_offsets_host"] == [0, 3, 3, 5] and p["obstacle_polar"].tolist() == [1, 0, 1, 0, 0]
    r = replicate(b, 3)
    assert r["obstacle_offsets_host"] == [0, 3] and r["obstacle_polar"].tolist() == [1, 0, 1] and r["n_decoys"] == 3
    with pytest.raises(ValueError, match="3 positions, 2 elements"):
        protein_to_batch(protein("c24"), obstacles=dict(ob, element=["N", "O"]))


# ---- recovery --------------------------------------------------------------------------------------------------------------------------------
def test_polar_recovery_on_hand_made_lists():
    from packppi_amd.functional import polar_recovery
    L = 3
    native = -torch.ones(2, L, 14, 4, dtype=torch.int32)
    sampled = native.clone()

    def bond(t, seg, a, b, both=True):
        for x, y in ((a, b), (b, a)) if both else ((a, b),):
            row, slot = divmod(x, 14)
            k = int((t[seg, row, slot] >= 0).sum())
            t[seg, row, slot, k] = y
    # segment 0: three native side-chain bonds, one backbone bond; the sample keeps two (one listed from one side only), adds one
    bond(native, 0, 0 * 14 + 5, 1 * 14 + 3)
    bond(native, 0, 0 * 14 + 6, 2 * 14 + 7)
    bond(native, 0, 1 * 14 + 4, 2 * 14 + 0)
    bond(native, 0, 0 * 14 + 0, 2 * 14 + 3)
    bond(sampled, 0, 0 * 14 + 5, 1 * 14 + 3)
    bond(sampled, 0, 2 * 14 + 7, 0 * 14 + 6, both=False)
    bond(sampled, 0, 0 * 14 + 0, 2 * 14 + 3)
    bond(sampled, 0, 1 * 14 + 9, 2 * 14 + 3)
    # segment 1: the same codes as a kept bond of segment 0, present in the native only
    bond(native, 1, 0 * 14 + 5, 1 * 14 + 3)
    n, k = polar_recovery(native, sampled)
    assert n.tolist() == [3, 1] and k.tolist() == [2, 0] and n.dtype == torch.int64
    # packed: the same rows as one [1, 6] array with a table
    n2, k2 = polar_recovery(native.reshape(1, 6, 14, 4), sampled.reshape(1, 6, 14, 4), seg_offsets=[0, 3, 6])
    assert n2.tolist() == [3, 1] and k2.tolist() == [2, 0]
    # an atom at the cap: its fifth bond is known from the partner's list
    cap_n = -torch.ones(1, 7, 14, 4, dtype=torch.int32)
    for j in range(1, 6):
        bond(cap_n, 0, 0 * 14 + 5, j * 14 + 0, both=False) if j < 5 else None
        bond(cap_n, 0, j * 14 + 0, 0 * 14 + 5, both=False)
    n3, k3 = polar_recovery(cap_n, cap_n)
    assert n3.tolist() == [5] and k3.tolist() == [5]
    n4, k4 = polar_recovery(dict(partners=native), dict(partners=native))
    assert n4.tolist() == k4.tolist() == [3, 1]
    with pytest.raises(ValueError, match="same shape"):
        polar_recovery(native, sampled[:1])
    with pytest.raises(ValueError, match="same shape"):
        polar_recovery(dict(partners=None), sampled)


# ---- argument rules --------------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from packppi_amd.lib import Context
    me = types.SimpleNamespace(plan=types.SimpleNamespace(device=torch.device("cpu")), _t={"chain_indices": torch.zeros(4)},
                               n_obstacles=0, n_rows=4, B=1, L=4)
    call = lambda **kw: Context.polar(me, **kw)
    for kw in (dict(hb_max=0.0), dict(hb_max=-1.0), dict(hb_max=float("nan")), dict(sb_max=float("inf")), dict(sb_max=0)):
        with pytest.raises(ValueError, match="finite and positive"):
            call(**kw)
    with pytest.raises(ValueError, match="bury_points"):
        call(bury_points=-1)
    with pytest.raises(ValueError, match="want_counts=True"):
        call(sasa=dict(area=torch.zeros(1, 4, 4), counts=None))
    with pytest.raises(ValueError, match="go together"):
        call(cls=torch.zeros(4, 14))
    with pytest.raises(ValueError, match="this context has 4 rows"):
        call(cls=torch.zeros(3, 14), ante=torch.zeros(3, 14, 2))
    with pytest.raises(ValueError, match="without obstacle atoms"):
        call(cls=torch.zeros(4, 14), ante=torch.zeros(4, 14, 2), obst_polar=torch.ones(3))
    me.n_obstacles = 5
    with pytest.raises(ValueError, match="holds 5 obstacle atoms"):
        call(cls=torch.zeros(4, 14), ante=torch.zeros(4, 14, 2), obst_polar=torch.ones(3))
    me._t = {}
    with pytest.raises(RuntimeError, match="chain_indices"):
        call()


def test_header_binding_and_build_list_name_the_export():
    import re
    from packppi_amd import build, lib
    hdr = open(os.path.join(os.path.dirname(GOLD), "..", "include", "packppi_hip.h")).read()
    assert re.search(r"pp_status pp_polar\(pp_ctx \*ctx,", hdr) and "#define PP_POLAR_CAP 4" in hdr
    assert "pp_polar" in lib.SYMBOLS and "pp_polar.hip" in build.sources_for(True) and "pp_polar.hip" in build.sources_for(False)
    assert O.CAP == 4
