"""CPU: anchors (pp_anchor_close) -- the definition's figures through tests/anchor_oracle.py, the host chemistry,
the LINK reader and writer, the spec parser, every refusal by name and the declarations the device side rests on.

The figures: on g0_protein_2FTL, three rows each of Cys, Ser, His, Asp, Glu, Met and Lys; a target 2.1 A from the donor of the
structure rebuilt at its own angles, at 120 degrees to its antecedent; sigma_d 0.1, sigma_theta 15.  Section 34 states Emin <= 0.292 on
every row, the 36^3 and 24^4 grids included; the bar here is Emin <= 1.0, in both precisions.  At every closed pick
|d - d0| <= sigma_d sqrt(Emin + 4) + the oracle tolerance, which follows from E <= thr."""
import functools
import os
import re
import warnings

import numpy as np
import pytest

from packppi_amd import constants as rc
from packppi_amd import pdb_io
from packppi_amd import selection as S

from . import anchor_oracle as O
from .conftest import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DONORS = {"CYS": "SG", "SER": "OG", "HIS": "NE2", "ASP": "OD1", "GLU": "OE1", "MET": "SD", "LYS": "NZ"}
D0, SD, TH0, ST = 2.1, 0.1, 120.0, 15.0


@functools.lru_cache(maxsize=None)
def protein():
    z = np.load(os.path.join(GOLD, "g0_protein_2FTL.npz"))
    return {k[5:]: z[k] for k in z.files if k.startswith("prot.")}


@functools.lru_cache(maxsize=None)
def host_batch():
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(protein())
    return {k: (v.numpy() if hasattr(v, "numpy") else v) for k, v in b.items()}


def native(hb, row):
    chi = hb["SC_D"].reshape(-1, 4)[row][None].astype(np.float64)
    return O._atoms(hb, row, chi, np.float64)[0] + hb["X"].reshape(-1, 14, 3)[row, 1].astype(np.float64)


@functools.lru_cache(maxsize=None)
def sites21():
    """The 21 rows' AnchorSet and the noisy start, 30 degrees off (seeded)."""
    hb = host_batch()
    rt, am = hb["residue_type"].reshape(-1), hb["atom_mask"].reshape(-1, 14)
    rng = np.random.default_rng(0)
    entries, seen = [], {}
    for r in range(rt.size):
        rn = rc.resnames[rt[r]]
        if rn not in DONORS or seen.get(rn, 0) >= 3 or not (am[r][np.asarray(rc.atom14_mask[rt[r]]) != 0] != 0).all():
            continue
        seen[rn] = seen.get(rn, 0) + 1
        slot = rc.atom14_names[rt[r]].index(DONORS[rn])
        ante = rc.anchor_antecedent(int(rt[r]), slot)
        q = O.place_target(native(hb, r), slot, ante, D0, TH0, float(rng.uniform(0, 2 * np.pi)))
        entries.append((r, slot, ante, q, (D0, SD, TH0, ST), f"{rn} {r}", "metal"))
    assert len(entries) == 21 and set(seen.values()) == {3}
    noise = np.deg2rad(30.0) * rng.standard_normal(hb["SC_D"].reshape(-1, 4).shape)
    start = (np.remainder(hb["SC_D"].reshape(-1, 4) + noise + np.pi, 2 * np.pi) - np.pi).astype(np.float32)
    return S.anchor_set_of(entries), start


@functools.lru_cache(maxsize=None)
def solved(dtype_name):
    a, start = sites21()
    hb = host_batch()
    return O.solve(hb, [0, hb["residue_type"].size], a, chi=start, dtype=np.dtype(dtype_name).type)


# ---- the figures of the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype_name", ["float32", "float64"])
def test_the_grids_reach_every_site(dtype_name):
    a, _ = sites21()
    r = solved(dtype_name)
    emin = np.array([float(r["emin"][int(row)]) for row in a.rows])
    ns = sorted({r["n"][int(row)] for row in a.rows})
    print(dtype_name, "Emin", emin.min(), emin.max(), "n", ns)
    assert ns == [1, 2, 3, 4]
    assert emin.max() <= 1.0 and (r["status"][a.rows] == 1).all() and r["count"].tolist() == [21]


def test_a_closed_pick_holds_the_distance():
    a, start = sites21()
    r32, r64 = solved("float32"), solved("float64")
    for row in (int(x) for x in a.rows):
        k = r32["pick"][row]
        tol = 4 * max(abs(float(r32["emin"][row]) - float(r64["emin"][row])), abs(float(r32["E"][row][k]) - float(r64["E"][row][k])),
                      abs(float(r32["D"][row][0, k]) - float(r64["D"][row][0, k])), abs(float(r32["ANG"][row][0, k]) - float(r64["ANG"][row][0, k])))
        assert 0 < tol < 5e-3
        d, emin = float(r32["report"][row, 2]), float(r32["report"][row, 0])
        assert abs(d - D0) <= SD * np.sqrt(emin + 4) + tol, (row, d, emin)
        n = r32["n"][row]
        assert np.array_equal(r32["chi"][row, n:].view(np.uint32), start[row, n:].view(np.uint32))
        assert not np.array_equal(r32["chi"][row, :n], start[row, :n])


def test_oracle_drops_what_the_definition_drops():
    hb = host_batch()
    a, start = sites21()
    row, slot, ante = int(a.rows[0]), int(a.slots[0]), int(a.antes[0])
    q, p = a.targets[0], a.params[0]
    bad = S.AnchorSet([row, row, -1, 10 ** 6, row, row, row, row], [slot, 4, slot, slot, slot, slot, slot, slot],
                      [slot, 1, ante, ante, ante, ante, ante, ante],
                      [q, q, q, q, [np.nan, 0, 0], q, q, q], [p, p, p, p, p, [D0, 0.0, TH0, ST], [D0, SD, np.inf, ST], p])
    assert O.valid(hb, bad).tolist() == [False] * 7 + [True]
    lists, marked = O.row_lists(hb, bad)
    assert lists == {row: [7]} and marked == {row}
    five = S.AnchorSet([row] * 5, [slot] * 5, [ante] * 5, [q] * 5, [p] * 5)
    lists, marked = O.row_lists(hb, five)
    assert lists == {row: [0, 1, 2, 3]} and marked == {row}


# ---- chemistry ----------------------------------------------------------------------------------------------------------------------------------
def test_chemistry_tables():
    assert rc.metal_distance("ZN", "N") == 2.1 and rc.metal_distance("zn", "O") == 2.1 and rc.metal_distance("FE", "S") == 2.3
    assert rc.metal_distance("CA", "O") == 2.4 and rc.metal_distance("NA", "O") == 2.4 and rc.metal_distance("K", "O") == 2.8
    assert rc.metal_distance("CA", "N") == 2.1
    with pytest.raises(ValueError, match="donor element"):
        rc.metal_distance("ZN", "C")
    assert {"ZN", "CA", "MG", "FE"} <= set(rc.metal_elements) and not set(rc.metal_elements) & set(rc.obstacle_radius)
    want = {("HIS", "ND1"): (126, 15), ("HIS", "NE2"): (126, 15), ("ASP", "OD2"): (120, 20), ("GLU", "OE1"): (120, 20), ("CYS", "SG"): (105, 12),
            ("MET", "SD"): (110, 15), ("SER", "OG"): (115, 15), ("THR", "OG1"): (115, 15), ("TYR", "OH"): (115, 15), ("LYS", "NZ"): (112, 12),
            ("ASN", "OD1"): (130, 20), ("GLN", "OE1"): (130, 20)}
    for (rn, atom), v in want.items():
        assert rc.anchor_angle[rn][atom] == v
        slot = rc.atom14_names[rc.resname_to_idx[rn]].index(atom)
        assert slot >= 5 and 4 <= rc.atom14_to_group[rc.resname_to_idx[rn], slot] <= 7          # every listed donor is one a chi moves
    assert (rc.ANCHOR_SIGMA_D_METAL, rc.ANCHOR_SIGMA_D_COVALENT, rc.PP_ANCHOR_PER_ROW) == (0.15, 0.10, 4)
    t = rc.resname_to_idx
    for rn, atom, ante in (("CYS", "SG", "CB"), ("HIS", "NE2", "CD2"), ("HIS", "ND1", "CG"), ("GLU", "OE1", "CD"), ("LYS", "NZ", "CE"), ("MET", "SD", "CG")):
        names = rc.atom14_names[t[rn]]
        assert names[rc.anchor_antecedent(t[rn], names.index(atom))] == ante
    assert abs(rc.covalent_radius["C"] + rc.covalent_radius["S"] - 1.81) < 1e-9


# ---- reading, writing, parsing ----------------------------------------------------------------------------------------------------------------
def hetatm(serial, name, resname, chain, resseq, xyz, element):
    shown = name.ljust(4) if len(element) == 2 or len(name) == 4 else f" {name}".ljust(4)
    return (f"HETATM{serial:>5} {shown} {resname:>3} {chain}{resseq:>4}    {xyz[0]:8.3f}{xyz[1]:8.3f}{xyz[2]:8.3f}{1.0:6.2f}{20.0:6.2f}"
            f"          {element:>2}").ljust(80)


@functools.lru_cache(maxsize=None)
def zinc_site():
    """(protein, his row, cys row, zinc position): a zinc 2.1 A from a deposited His NE2, in the ring plane, on the line from the
    midpoint of CD2 and CE1 through NE2 (about 126 degrees to either)."""
    prot = protein()
    aa = np.asarray(prot["aaindex"])
    full = [r for r in range(len(aa)) if (np.asarray(prot["atom_mask"])[r][np.asarray(rc.atom14_mask[aa[r]]) != 0] != 0).all()]
    his = [r for r in full if rc.resnames[aa[r]] == "HIS"][0]
    cys = [r for r in full if rc.resnames[aa[r]] == "CYS"][0]
    names = rc.atom14_names[rc.resname_to_idx["HIS"]]
    xyz = np.asarray(prot["atom_positions"], np.float64)[his]
    ne2, mid = xyz[names.index("NE2")], 0.5 * (xyz[names.index("CD2")] + xyz[names.index("CE1")])
    zn = ne2 + 2.1 * (ne2 - mid) / np.linalg.norm(ne2 - mid)
    return prot, his, cys, np.round(zn, 3)


def write_pdb(tmp_path, head, extra):
    prot = zinc_site()[0]
    path = tmp_path / "site.pdb"
    path.write_text(head + pdb_io.insert_obstacle_lines(pdb_io.to_pdb(prot), extra))
    return str(path)


def test_link_records_round_trip(tmp_path):
    prot, his, cys, zn = zinc_site()
    lig = np.asarray(prot["atom_positions"], np.float64)[cys, 5] + np.array([1.0, 1.0, 1.0])
    het = [hetatm(9001, "ZN", "ZN", "Z", 301, zn, "ZN"), hetatm(9002, "C1", "LIG", "Z", 302, lig, "C")]
    hetero = [dict(chain="Z", resseq=301, icode=" ", resname="ZN", name="ZN", element="ZN", xyz=np.float32(zn)),
              dict(chain="Z", resseq=302, icode=" ", resname="LIG", name="C1", element="C", xyz=np.float32(lig))]
    ch, num = prot["chain_id"], prot["residue_index"]
    spec = f"{ch[his]}:{int(num[his])}:NE2=Z:301:ZN, {ch[cys]}:{int(num[cys])}:SG=Z:302:C1"
    a = S.parse_anchors(spec, prot, hetero)
    assert a.rows.tolist() == [his, cys] and a.kinds == ["metal", "link"] and a.slots.tolist() == [9, 5]
    assert np.allclose(a.params[0], (2.1, 0.15, 126.0, 15.0)) and np.allclose(a.params[1], (1.81, 0.10, 105.0, 12.0))
    head = pdb_io.link_lines(prot, a, hetero, lengths=[2.1, 1.77])
    assert all(len(ln) == 80 for ln in head.splitlines()) and head.count("LINK") == 2
    path = write_pdb(tmp_path, head, het)
    recs = pdb_io.link_records(path)
    assert [(r["name1"], r["resname1"], r["chain1"], r["resseq1"], r["name2"], r["resname2"], r["chain2"], r["resseq2"], r["sym1"], r["sym2"],
             r["length"]) for r in recs] == [("NE2", "HIS", str(ch[his]), int(num[his]), "ZN", "ZN", "Z", 301, "1555", "1555", 2.1),
                                             ("SG", "CYS", str(ch[cys]), int(num[cys]), "C1", "LIG", "Z", 302, "1555", "1555", 1.77)]
    assert [(h["name"], h["element"]) for h in pdb_io.hetero_atoms(path)] == [("ZN", "ZN"), ("C1", "C")]
    back = pdb_io.anchor_sites(path, prot, "link")
    assert back.rows.tolist() == a.rows.tolist() and back.slots.tolist() == a.slots.tolist() and back.antes.tolist() == a.antes.tolist()
    assert np.allclose(back.targets, a.targets, atol=1e-3) and back.kinds == a.kinds and back.labels == [t.strip() for t in spec.split(",")]
    assert np.allclose(back.params[0], a.params[0]) and np.allclose(back.params[1], (1.77, 0.10, 105.0, 12.0))      # the record's distance column
    # a distance column outside 1.2 .. 2.0 A: the sum of the covalent radii
    path = write_pdb(tmp_path, pdb_io.link_lines(prot, a, hetero, lengths=[2.1, 2.4]), het)
    assert np.allclose(pdb_io.anchor_sites(path, prot, "link").params[1], (1.81, 0.10, 105.0, 12.0))


def test_link_mode_skips_protein_links_and_symmetry_mates(tmp_path):
    prot, his, cys, zn = zinc_site()
    hetero = [dict(chain="Z", resseq=301, icode=" ", resname="ZN", name="ZN", element="ZN", xyz=np.float32(zn))]
    a = S.parse_anchors(f"{prot['chain_id'][his]}:{int(prot['residue_index'][his])}:NE2=Z:301:ZN", prot, hetero)
    good = pdb_io.link_lines(prot, a, hetero)
    mate = good[:59] + "  2555" + good[65:]
    ch, num = prot["chain_id"], prot["residue_index"]
    pp = (f"LINK         SG  CYS {ch[cys]}{int(num[cys]):>4}".ljust(42) + f" NE2 HIS {ch[his]}{int(num[his]):>4}").ljust(59) + "  1555   1555"
    path = write_pdb(tmp_path, good + mate + pp.ljust(80) + "\n", [hetatm(9001, "ZN", "ZN", "Z", 301, zn, "ZN")])
    assert len(pdb_io.link_records(path)) == 3
    said = []
    back = pdb_io.anchor_sites(path, prot, "link", log=said.append)
    assert len(back) == 1 and back.rows.tolist() == [his]
    assert len(said) == 2 and any("two protein residues" in m for m in said) and any("symmetry mate" in m for m in said)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        pdb_io.anchor_sites(path, prot, "link")
    assert len(w) == 2
    with pytest.raises(ValueError, match="mode must be one of"):
        pdb_io.anchor_sites(path, prot, "backbone")


def test_geometry_mode_finds_exactly_the_synthesised_donors(tmp_path):
    prot, his, cys, zn = zinc_site()
    ca = np.asarray(prot["atom_positions"], np.float64)[his, 1] + 40.0          # a sodium far from everything: no donor
    path = write_pdb(tmp_path, "", [hetatm(9001, "ZN", "ZN", "Z", 301, zn, "ZN"), hetatm(9002, "NA", "NA", "Z", 302, ca, "NA"),
                                    hetatm(9003, "C1", "LIG", "Z", 303, zn + 0.5, "C")])
    a = pdb_io.anchor_sites(path, prot, "geometry")
    assert a.rows.tolist() == [his] and a.slots.tolist() == [9] and a.kinds == ["metal"]
    assert np.allclose(a.targets[0], zn, atol=1e-3) and np.allclose(a.params[0], (2.1, 0.15, 126.0, 15.0))
    assert "IN THE DEPOSITED COORDINATES" in pdb_io.anchor_sites.__doc__ and "never where" in pdb_io.anchor_sites.__doc__
    assert len(pdb_io.anchor_sites(path, prot, "link")) == 0                      # no LINK record, no anchor


def test_geometry_mode_keeps_four_contacts_per_residue(tmp_path):
    """An Asp whose two oxygens see three metals finds six contacts: the four nearest their ideal distance stay, one warning names the rest."""
    prot = zinc_site()[0]
    aa, xyz = np.asarray(prot["aaindex"]), np.asarray(prot["atom_positions"], np.float64)
    asp = [r for r in range(len(aa)) if rc.resnames[aa[r]] == "ASP" and np.asarray(prot["atom_mask"])[r, :8].all()][0]
    cb, cg = xyz[asp, 4], xyz[asp, 5]
    u = (cg - cb) / np.linalg.norm(cg - cb)
    het = [hetatm(9001 + k, "ZN", "ZN", "Z", 301 + k, np.round(cg + t * u, 3), "ZN") for k, t in enumerate((2.2, 2.3, 2.4))]
    path = write_pdb(tmp_path, "", het)
    said = []
    a = pdb_io.anchor_sites(path, prot, "geometry", log=said.append)
    mine = [i for i in range(len(a)) if a.rows[i] == asp]
    assert len(mine) == 4 and {rc.atom14_names[aa[asp]][a.slots[i]] for i in mine} == {"OD1", "OD2"}
    assert len(said) == 1 and "more than 4" in said[0] and said[0].count("=Z:") == 2
    hb = host_batch()
    S.check_anchor_set(a.subset(mine), hb["residue_type"].reshape(-1), hb["residue_mask"].reshape(-1), hb["atom_mask"].reshape(-1, 14),
                       [0, len(aa)])                                       # what is left passes the check that refuses a fifth


def test_pinned_holds_closed_kept_and_dropped_rows():
    import torch
    from packppi_amd.lib import AnchorResult
    res = AnchorResult(status=torch.tensor([0, 1, 2, -1, -2], dtype=torch.int32))
    assert res.pinned().tolist() == [False, True, True, False, True]      # a row of status -2 may have been closed by its other anchors
    with pytest.raises(RuntimeError, match="dropped"):
        res.closed()
    assert AnchorResult(status=torch.tensor([0, 1, 2, -1], dtype=torch.int32)).closed() == [1]


def test_parse_anchors_refuses_by_name():
    prot, his, cys, zn = zinc_site()
    hetero = [dict(chain="Z", resseq=301, icode=" ", resname="ZN", name="ZN", element="ZN", xyz=np.float32(zn)),
              dict(chain="Z", resseq=302, icode=" ", resname="XE", name="XE", element="XE", xyz=np.float32(zn))]
    c, n = prot["chain_id"][his], int(prot["residue_index"][his])
    for spec, msg in (("", "empty anchor list"), ("A:94=Z:301:ZN", "expected CHAIN:N:ATOM=CHAIN:N:ATOM"), (f"?:{n}:NE2=Z:301:ZN", "no residue"),
                      (f"{c}:{n}:NE2=Z:999:ZN", "0 hetero atoms match"), (f"{c}:{n}:CB=Z:301:ZN", "no side-chain atom CB beyond CB"),
                      (f"{c}:{n}:QQ=Z:301:ZN", "no side-chain atom QQ"), (f"{c}:{n}:NE2=Z:302:XE", "no covalent radius")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            S.parse_anchors(spec, prot, hetero)


# ---- refusals of the set, by name ----------------------------------------------------------------------------------------------------------------
def test_check_anchor_set_refuses_by_name():
    hb = host_batch()
    rt, rm, am = hb["residue_type"].reshape(-1), hb["residue_mask"].reshape(-1), hb["atom_mask"].reshape(-1, 14)
    a, _ = sites21()
    N = rt.size
    offs = [0, 100, N]
    assert S.check_anchor_set(a, rt, rm, am, [0, N]) is a
    row, slot, ante, q, p = int(a.rows[0]), int(a.slots[0]), int(a.antes[0]), a.targets[0], a.params[0]

    def one(**kw):
        d = dict(rows=[row], slots=[slot], antes=[ante], targets=[q], params=[p], labels=["Zn site"])
        d.update(kw)
        return S.AnchorSet(**d)
    gly = int(np.nonzero(rt == rc.resname_to_idx["GLY"])[0][0])
    am2 = am.copy()
    am2[row, slot] = 0
    rm2 = rm.copy()
    rm2[row] = 0
    cases = [(one(rows=[N]), (rt, rm, am), "anchor Zn site: row %d is outside" % N),
             (one(rows=[-1]), (rt, rm, am), "is outside"),
             (one(), (rt, rm2, am), "anchor Zn site: row %d is masked out" % row),
             (one(slots=[4]), (rt, rm, am), "slot 4 of row %d is no side-chain atom that a chi angle moves" % row),
             (one(rows=[gly], slots=[5]), (rt, rm, am), "is no side-chain atom"),
             (one(antes=[slot]), (rt, rm, am), "antecedent slot %d" % slot),
             (one(antes=[14]), (rt, rm, am), "antecedent slot 14"),
             (one(), (rt, rm, am2), "row %d lacks %s" % (row, rc.atom14_names[rt[row]][slot])),
             (one(targets=[[np.nan, 0, 0]]), (rt, rm, am), "must be finite"),
             (one(params=[[D0, 0.0, TH0, ST]]), (rt, rm, am), "sigma_d positive"),
             (one(params=[[D0, SD, np.inf, ST]]), (rt, rm, am), "must be finite"),
             (S.AnchorSet([row] * 5, [slot] * 5, [ante] * 5, [q] * 5, [p] * 5), (rt, rm, am), "the fifth anchor on row %d" % row)]
    for s, arrays, msg in cases:
        with pytest.raises(ValueError, match=re.escape(msg)):
            S.check_anchor_set(s, *arrays, [0, N])
    with pytest.raises(ValueError, match=re.escape("CYS 41 lies in segment")):
        S.check_anchor_set(one(labels=[""]).shifted(0, 1 if row < 100 else 0), rt, rm, am, offs, names={row: "CYS 41"})
    assert S.check_anchor_set(one().shifted(0, 0 if row < 100 else 1), rt, rm, am, offs) is not None


def test_anchor_set_rules():
    a, _ = sites21()
    with pytest.raises(ValueError, match="AnchorSet: 1 slots for 2 rows"):
        S.AnchorSet([1, 2], [5], [4, 4], np.zeros((2, 3)), np.ones((2, 4)))
    assert len(S.AnchorSet()) == 0 and len(S.AnchorSet.concat([])) == 0
    sh = a.shifted(7, 3)
    assert sh.rows.tolist() == (a.rows + 7).tolist() and sh.segment == 3 and a.segment is None and sh.labels == a.labels
    both = S.AnchorSet.concat([a, sh])
    assert len(both) == 42 and both.segment is None and both.rows[21:].tolist() == sh.rows.tolist()
    assert a.targets.dtype == np.float32 and a.params.shape == (21, 4) and a.rows.dtype == np.int32


# ---- the module's refusals ----------------------------------------------------------------------------------------------------------------------
def test_module_refusals_and_row_shifts():
    from packppi_amd import synth
    from packppi_amd.batch import collate, pack
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.module import _anchor_refusals
    parts = [protein_to_batch(synth.make_complex(20, 3)), protein_to_batch(synth.make_complex(17, 4))]
    one = S.AnchorSet([3], [5], [4], [[0, 0, 0]], [[D0, SD, TH0, ST]], labels=["x"])
    packed = pack(parts)
    sets, auto = _anchor_refusals(packed, [one, one], False, False)
    assert not auto and [s.rows.tolist() for s in sets] == [[3], [23]] and [s.segment for s in sets] == [0, 1]
    sets, _ = _anchor_refusals(packed, [None, one], False, False)
    assert sets[0] is None and sets[1].rows.tolist() == [23]
    sets, _ = _anchor_refusals(parts[0], one, False, False)
    assert sets[0].rows.tolist() == [3] and sets[0].segment == 0
    import torch
    padded = collate([{**{k: (v[0] if isinstance(v, torch.Tensor) else v) for k, v in p.items()}, "num_nodes": n} for p, n in zip(parts, (20, 17))])
    for batch, val, kw, msg in ((padded, one, {}, "not a padded B > 1 batch"), (packed, [one, one], dict(rt=True), "return_trajectory with anchors"),
                                (packed, [one, one], dict(rl=True), "return_list with anchors"), (packed, [one], {}, "holds 1 sets, the batch holds 2"),
                                (packed, one, {}, "holds 1 sets, the batch holds 2"), (packed, 7, {}, "anchors must be None"),
                                (packed, [one, "x"], {}, "anchors must be None"), (packed, "auto", {}, "needs batch.pdb_path"),
                                (parts[0], "A:1:SG=Z:1:ZN", {}, "needs batch.pdb_path")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            _anchor_refusals(batch, val, kw.get("rt", False), kw.get("rl", False))
    from packppi_amd.batch import Batch
    with pytest.raises(ValueError, match="needs batch.residue_names"):
        _anchor_refusals(Batch(parts[0], pdb_path="site.pdb"), "auto", False, False)


def test_command_line_flag_and_csv():
    from packppi_amd.cli import eval_diffusion as E
    from packppi_amd.cli import proximal_optimize as P
    base = ["--input", "x.pdb", "--outdir", "o", "--molprobity_clash_loc", "m"]
    assert not hasattr(E.parse_args(base), "anchors") and not hasattr(P.parse_args(base), "anchors")      # the namespace as before
    assert E.parse_args(base + ["--anchors", "auto"]).anchors == "auto" and P.parse_args(base + ["--anchors", "geometry"]).anchors == "geometry"
    assert E.anchors_from_args(E.parse_args(base)) is None and E.anchors_from_args(E.parse_args(base + ["--anchors", " auto "])) == "auto"
    with pytest.raises(SystemExit):
        E.parse_args(base + ["--anchors", "auto", "--seed", "1", "--n_decoys", "4"])
    prot, his, cys, zn = zinc_site()
    hetero = [dict(chain="Z", resseq=301, icode=" ", resname="ZN", name="ZN", element="ZN", xyz=np.float32(zn))]
    a = S.parse_anchors(f"{prot['chain_id'][his]}:{int(prot['residue_index'][his])}:NE2=Z:301:ZN", prot, hetero)
    n = len(prot["aaindex"])
    status, report = [0] * n, [[0.0] * 4 for _ in range(n)]
    status[his], report[his] = 1, [0.25, 0.5, 2.11, 125.0]
    text = E.anchors_csv(prot, a, status, report, [[2.11, 125.0]], [[3.4, 90.0]])
    lines = text.splitlines()
    assert lines[0] == "chain,number,atom,target,kind,d0,distance_before,distance_after,angle,energy,status" and len(lines) == 2
    assert lines[1] == f"{prot['chain_id'][his]},{int(prot['residue_index'][his])},NE2,Z:301:ZN,metal,2.100,3.4000,2.1100,125.00,0.5000,closed"


# ---- what the device side rests on --------------------------------------------------------------------------------------------------------------
def test_the_header_and_the_source_carry_the_definition():
    hdr = re.sub(r"[\s*/]+", " ", open(os.path.join(ROOT, "include", "packppi_hip.h")).read())
    src = re.sub(r"[\s*/]+", " ", open(os.path.join(ROOT, "packppi_amd", "csrc", "pp_anchor.hip")).read())
    for sentence in ("A row may carry at most PP_ANCHOR_PER_ROW = 4 anchors. They are taken in list order.",
                     "the rigid group of slot (a2g) is a chi group, 4..7 (CB never moves)",
                     "An invalid entry, or a fifth anchor on a row, is dropped on the device and the row's status becomes -2.",
                     "The Python layer refuses it by name before the call.",
                     "n = the largest (group - 3) over the row's valid anchors",
                     "g(n) = 72, 72, 36, 24.", "theta_k = (float)(-pi + 2 pi k / g).", "A NaN never wins a minimum.",
                     "thr = max(Emin, min(max_energy, Emin + 4)) and F = {E <= thr}.",
                     "The pick is the argmin of J over F, ties to the lowest flat index.",
                     "A fixed row is kept: status 2.", "Each row's result is a function of that row's data and its anchors only."):
        s = re.sub(r"[\s*/]+", " ", sentence)
        assert s in hdr, sentence
        assert s in src, sentence
    assert "#define PP_ANCHOR_PER_ROW 4" in open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    proto = re.search(r"pp_status pp_anchor_close\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "packppi_hip.h")).read(), flags=re.S))
    args = [x.strip().split()[-1].lstrip("*") for x in proto.group(1).split(",")]
    assert args == ["ctx", "chi", "fixed", "anchors_i", "anchors_target", "anchors_param", "A", "max_energy", "sigma_chi", "chi_out", "status",
                    "report", "anchor_report", "count", "stream"]


def test_the_library_builds_and_binds_the_entry():
    from packppi_amd import build, lib
    assert "pp_anchor.hip" in build.sources_for(True) and "pp_anchor.hip" in build.sources_for(False)
    assert "pp_anchor_close" in lib.SYMBOLS
    assert callable(lib.Context.anchors) and callable(lib.Context.check_anchors)
    from packppi_amd import functional
    assert callable(functional.close_anchors)
    src = open(os.path.join(ROOT, "packppi_amd", "csrc", "pp_anchor.hip")).read()
    assert "atomicAdd(" not in src and "PP_WS_ANCHOR" in src and "#pragma clang fp contract(off)" in src
