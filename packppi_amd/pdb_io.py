"""PDB text <-> protein dict, without Biopython.

Read side reproduces what ``from_pdb_file``/``from_pdb_string`` (src/utils/protein.py:55-199)
obtain through Biopython 1.84's permissive ``PDBParser``: only ``ATOM`` records; chains
sorted by id; residues stably sorted by sequence number; alternate locations resolved to
the highest occupancy (first wins ties); a repeated atom name keeps its first record;
non-standard residues and atoms outside the residue's atom14 slots (all hydrogens) are
dropped; insertion codes shift later indices by one each; duplicate indices inside a
chain are bumped.  Biopython itself is not in this image, so this step is
**parity-unpinned**  -- everything downstream of the dict is pinned.

Write side reproduces ``to_pdb`` (protein.py:207-314) column for column.
"""
import gzip
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

from . import constants as rc


def _atom_records(path) -> List[str]:
    path = str(path)
    if path.endswith("pdb.gz"):
        with gzip.open(path, "rb") as fh:
            raw = [ln.decode() for ln in fh]
    elif path.endswith("pdb"):
        with open(path, "r") as fh:
            raw = list(fh)
    else:
        raise ValueError("Unrecognized file type.")
    return [ln.strip() for ln in raw if ln.startswith("ATOM")]


def parse_atom_records(lines: List[str], mse_to_met: bool = True, ignore_non_std: bool = True) -> Dict:
    # chain -> ordered list of residues; residue = dict(resseq, icode, resname, atoms{name: [occ, xyz, b]})
    chains: Dict[str, List[dict]] = {}
    by_id: Dict[tuple, dict] = {}
    for ln in lines:
        ln = ln.ljust(80)
        fullname = ln[12:16]
        parts = fullname.split()
        name = parts[0] if len(parts) == 1 else fullname
        altloc = ln[16]
        resname = ln[17:20].strip()
        chain_id = ln[21]
        try:
            resseq = int(ln[22:26].split()[0])
            xyz = (float(ln[30:38]), float(ln[38:46]), float(ln[46:54]))
        except (ValueError, IndexError):
            continue
        icode = ln[26]
        try:
            occ = float(ln[54:60])
        except ValueError:
            occ = None
        try:
            bfac = float(ln[60:66])
        except ValueError:
            bfac = 0.0
        key = (chain_id, resseq, icode)
        res = by_id.get(key)
        if res is None or res["resname"] != resname:
            if res is not None:
                # same id, different residue name (point-mutation microheterogeneity): keep the first
                continue
            res = dict(resseq=resseq, icode=icode, resname=resname, atoms={})
            by_id[key] = res
            chains.setdefault(chain_id, []).append(res)
        slot = res["atoms"].get(name)
        occ_cmp = -1.0 if occ is None else occ
        if slot is None:
            res["atoms"][name] = [occ_cmp, np.float32(xyz), bfac, altloc != " "]
        elif altloc != " " and slot[3] and occ_cmp > slot[0]:
            res["atoms"][name] = [occ_cmp, np.float32(xyz), bfac, True]
        # else: atom defined twice / lower-or-equal occupancy altloc -> first record stays

    pos_l, aa_l, mask_l, idx_l, chain_l, bf_l = [], [], [], [], [], []
    icode_shift = 0
    for cid in sorted(chains):
        for res in sorted(chains[cid], key=lambda r: r["resseq"]):
            resname, atoms = res["resname"], res["atoms"]
            if resname == "HOH":
                continue
            if mse_to_met and resname == "MSE":
                resname = "MET"
                if "SE" in atoms:
                    atoms = {("SD" if k == "SE" else k): v for k, v in atoms.items()}
            rt = rc.resname_to_idx.get(resname, 20)
            if rt == 20:
                if ignore_non_std:
                    continue
            if res["icode"] != " ":
                icode_shift += 1
            names = rc.atom14_names[rt]
            pos = np.full((14, 3), np.nan)
            mask = np.zeros(14)
            bf = np.zeros(14)
            for aname, (_, xyz, b, _) in atoms.items():
                if aname and aname in names:
                    k = names.index(aname)
                    pos[k], mask[k], bf[k] = xyz, 1.0, b
            if mask.sum() < 0.5:
                continue
            pos_l.append(pos); aa_l.append(rt); mask_l.append(mask)
            idx_l.append(res["resseq"] + icode_shift); chain_l.append(cid); bf_l.append(bf)

    used: Dict[str, set] = {}
    new_idx = []
    for cid, idx in zip(chain_l, idx_l):
        taken = used.setdefault(cid, set())
        while idx in taken:
            idx += 1
        taken.add(idx)
        new_idx.append(idx)

    return dict(atom_positions=np.array(pos_l), atom_mask=np.array(mask_l), aaindex=np.array(aa_l),
                residue_index=np.array(new_idx), chain_id=np.array(chain_l), b_factors=np.array(bf_l))


def from_pdb_file(pdb_file, mse_to_met: bool = True) -> Dict:
    return parse_atom_records(_atom_records(Path(pdb_file)), mse_to_met=mse_to_met)


_WATERS = ("HOH", "WAT", "DOD")


def _raw_lines(path) -> List[str]:
    path = str(path)
    if path.endswith("pdb.gz"):
        with gzip.open(path, "rb") as fh:
            return [ln.decode() for ln in fh]
    if path.endswith("pdb"):
        with open(path, "r") as fh:
            return list(fh)
    raise ValueError("Unrecognized file type.")


def _element(ln: str) -> str:
    """Element of an ATOM / HETATM record: columns 77-78; if blank, the leading letters of the name field by the PDB alignment rule
    (a one-letter element's name starts in column 14, a two-letter element's in column 13)."""
    el = ln[76:78].strip().upper()
    if el:
        return el
    field = ln[12:16]
    if field[0].isalpha() and not (field[0] == "H" and len(field.strip()) == 4):
        return field[:2].strip().upper()
    letters = [c for c in field if c.isalpha()]
    return letters[0].upper() if letters else ""


def obstacle_atoms(pdb_file, water: bool = False, mse_to_met: bool = True, log=None) -> Dict:
    """The atoms of a PDB file that ``from_pdb_file`` does not return and that side chains must not overlap:
    every ``HETATM`` record and every ``ATOM`` record of a residue the protein dict drops as non-standard (after MSE -> MET) --
    ligands, cofactors, nucleic acids, modified residues.  Alternate locations are resolved by the protein rule (highest occupancy,
    the first record wins ties; a repeated atom keeps its first record).  Skipped: hydrogens and deuterium; waters (HOH, WAT, DOD)
    unless ``water``; any element without a radius in ``constants.obstacle_radius`` (metals: coordination is not a clash), named
    once in a warning (``log``, default ``warnings.warn``).

    Returns ``dict(xyz [M, 3] float32, radius [M] float32, element, resname, chain, resseq (lists of M), lines)``.  ``lines`` is
    for writing the groups back as deposited: the original line, without the newline, of every record of the groups read here
    (waters only with ``water``), in file order -- their hydrogens, radius-less atoms and every alternate location included, so
    that a written structure carries the whole ligand, not only the atoms that act as obstacles."""
    kept: Dict[tuple, list] = {}           # (chain, resseq, icode, resname, atom name) -> [occ, has altloc, line, element, xyz]
    order: List[tuple] = []
    skipped = set()
    lines: List[str] = []
    for raw in _raw_lines(Path(pdb_file)):
        het = raw.startswith("HETATM")
        if not het and not raw.startswith("ATOM"):
            continue
        line = raw.rstrip("\r\n")
        ln = line.ljust(80)
        resname = ln[17:20].strip()
        if not het:
            std = "MET" if (mse_to_met and resname == "MSE") else resname
            if rc.resname_to_idx.get(std, 20) != 20:
                continue                                   # a standard residue: the protein dict has it
        if resname in _WATERS and not water:
            continue
        lines.append(line)
        el = _element(ln)
        if el in ("H", "D"):
            continue
        try:
            resseq = int(ln[22:26].split()[0])
            xyz = (float(ln[30:38]), float(ln[38:46]), float(ln[46:54]))
        except (ValueError, IndexError):
            continue
        if el not in rc.obstacle_radius:
            skipped.add(el or "?")
            continue
        try:
            occ = float(ln[54:60])
        except ValueError:
            occ = -1.0
        altloc = ln[16]
        key = (ln[21], resseq, ln[26], resname, ln[12:16])
        slot = kept.get(key)
        if slot is None:
            kept[key] = [occ, altloc != " ", line, el, xyz]
            order.append(key)
        elif altloc != " " and slot[1] and occ > slot[0]:
            kept[key] = [occ, True, line, el, xyz]
    if skipped:
        msg = ("obstacle_atoms: no van der Waals radius for element(s) " + ", ".join(sorted(skipped)) + " in " + str(pdb_file) +
               ": those atoms are not obstacles")
        if log is not None:
            log(msg)
        else:
            import warnings
            warnings.warn(msg)
    recs = [kept[k] for k in order]
    return dict(xyz=np.array([r[4] for r in recs], np.float32).reshape(-1, 3),
                radius=np.array([rc.obstacle_radius[r[3]] for r in recs], np.float32),
                element=[r[3] for r in recs], resname=[k[3] for k in order], chain=[k[0] for k in order],
                resseq=[k[1] for k in order], lines=lines)


OBSTACLE_MODES = ("none", "hetero", "hetero+water")


def obstacles_for(pdb_file, mode: str, log=print):
    """The ``--obstacles`` flag of the command lines: None for "none", else ``obstacle_atoms`` (with the waters for "hetero+water")."""
    if mode not in OBSTACLE_MODES:
        raise ValueError(f"obstacles must be one of {OBSTACLE_MODES}")
    if mode == "none":
        return None
    o = obstacle_atoms(pdb_file, water=mode == "hetero+water", log=log)
    log(f"----- {len(o['radius'])} obstacle atoms ({mode}) from {len(o['lines'])} records; the network does not see them -----")
    return o


def insert_obstacle_lines(pdb_text: str, lines: List[str]) -> str:
    """``to_pdb`` output with the obstacle records' original lines, verbatim, between the protein's last TER and END."""
    if not lines:
        return pdb_text
    out = pdb_text.split("\n")
    at = max(i for i, ln in enumerate(out) if ln.startswith("TER")) + 1
    return "\n".join(out[:at] + list(lines) + out[at:])


def ssbond_records(prot: Dict, pairs, lengths=None) -> str:
    """The SSBOND records of the row pairs ``pairs`` of ``prot`` (80 columns each, serial numbers from 1, symmetry 1555, the bond
    length from ``lengths`` if given): the text that goes in front of ``to_pdb(prot)``."""
    out = []
    for k, (a, b) in enumerate(pairs):
        ends = "".join(f"CYS {str(prot['chain_id'][r])[:1]} {int(prot['residue_index'][r]):>4d}" + ("    " if i == 0 else "")
                       for i, r in enumerate((a, b)))
        ln = f"SSBOND {k + 1:>3d} {ends}".ljust(59) + f"{1555:>6d} {1555:>6d}"
        if lengths is not None:
            ln += f" {float(lengths[k]):5.2f}"
        out.append(ln.ljust(80) + "\n")
    return "".join(out)


def hetero_atoms(pdb_file, mse_to_met: bool = True) -> List[Dict]:
    """Every atom of a PDB file that the protein dict does not hold and that an anchor can point at: the
    ``HETATM`` records and the ``ATOM`` records of non-standard residues, metals included, without waters and hydrogens; the first
    record of an atom wins.  One dict per atom: ``chain``, ``resseq``, ``icode``, ``resname``, ``name``, ``element``, ``xyz``."""
    out, seen = [], set()
    for raw in _raw_lines(Path(pdb_file)):
        het = raw.startswith("HETATM")
        if not het and not raw.startswith("ATOM"):
            continue
        ln = raw.rstrip("\r\n").ljust(80)
        resname = ln[17:20].strip()
        if not het and rc.resname_to_idx.get("MET" if (mse_to_met and resname == "MSE") else resname, 20) != 20:
            continue
        el = _element(ln)
        if resname in _WATERS or el in ("H", "D"):
            continue
        try:
            resseq = int(ln[22:26].split()[0])
            xyz = np.float32((float(ln[30:38]), float(ln[38:46]), float(ln[46:54])))
        except (ValueError, IndexError):
            continue
        key = (ln[21], resseq, ln[26], resname, ln[12:16].strip())
        if key in seen:
            continue
        seen.add(key)
        out.append(dict(chain=ln[21], resseq=resseq, icode=ln[26], resname=resname, name=ln[12:16].strip(), element=el, xyz=xyz))
    return out


def link_records(pdb_file) -> List[Dict]:
    """The LINK records of a PDB file by their fixed columns: one dict per record with ``name1``, ``altloc1``, ``resname1``,
    ``chain1``, ``resseq1``, ``icode1``, the same with 2, ``sym1``, ``sym2`` (text, "" if blank) and ``length`` (float or None).  A
    record whose residue numbers do not parse is left out."""
    out = []
    for raw in _raw_lines(Path(pdb_file)):
        if not raw.startswith("LINK  "):
            continue
        ln = raw.rstrip("\r\n").ljust(80)
        try:
            seq1, seq2 = int(ln[22:26]), int(ln[52:56])
        except ValueError:
            continue
        try:
            length = float(ln[73:78])
        except ValueError:
            length = None
        out.append(dict(name1=ln[12:16].strip(), altloc1=ln[16].strip(), resname1=ln[17:20].strip(), chain1=ln[21], resseq1=seq1,
                        icode1=ln[26].strip(), name2=ln[42:46].strip(), altloc2=ln[46].strip(), resname2=ln[47:50].strip(),
                        chain2=ln[51], resseq2=seq2, icode2=ln[56].strip(), sym1=ln[59:65].strip(), sym2=ln[66:72].strip(),
                        length=length))
    return out


ANCHOR_MODES = ("link", "geometry")


def anchor_sites(pdb_file, protein: Dict, mode: str = "link", log=None):
    """The ``selection.AnchorSet`` of a PDB file's metal sites and covalent links.

    ``"link"``: every LINK record between a side-chain atom (atom14 slot >= 5) of a standard residue of ``protein`` and a HETATM or
    non-standard-residue atom present in the file, with an identity (1555) or blank symmetry operator on both sides.  The target is
    that atom's coordinates.  A metal target takes ``constants.metal_distance``; for a covalent link d0 is the record's distance
    column when it lies in 1.2 to 2.0 A, else the sum of the covalent radii.  Protein-protein LINKs and symmetry mates are skipped with
    one warning each (``log``, default ``warnings.warn``).

    ``"geometry"``: metals only.  A donor atom (N, O or S of the residues in ``constants.anchor_angle``) within d0 + 0.5 A of a metal
    IN THE DEPOSITED COORDINATES of ``protein`` becomes an anchor.  The input's side chains decide WHICH atoms coordinate, never where
    they go: the anchor holds the metal's position and the ideal distance and angle, not the deposited donor position.  A structure
    without side chains has no donors to find; nothing detects anchors from the backbone alone.  A residue that finds more than four
    contacts (a carboxylate next to a metal cluster) keeps the four nearest their ideal distance; the others are named in one warning."""
    from .selection import anchor_entry, anchor_set_of
    if mode not in ANCHOR_MODES:
        raise ValueError(f"anchors: mode must be one of {ANCHOR_MODES}")

    def warn(msg):
        if log is not None:
            log(msg)
        else:
            import warnings
            warnings.warn(msg)

    het = hetero_atoms(pdb_file)
    chain_id = np.asarray(protein["chain_id"])
    number = np.asarray(protein["residue_index"]).astype(np.int64)
    aa = np.asarray(protein["aaindex"])
    entries = []
    if mode == "geometry":
        xyz, amask = np.asarray(protein["atom_positions"], np.float64), np.asarray(protein["atom_mask"])
        for h in het:
            if h["element"] not in rc.metal_elements:
                continue
            for r in range(len(aa)):
                table = rc.anchor_angle.get(rc.resnames[int(aa[r])], {})
                for atom in table:
                    slot = rc.atom14_names[int(aa[r])].index(atom)
                    d0 = rc.metal_distance(h["element"], atom[0])
                    dist = np.linalg.norm(xyz[r, slot] - np.asarray(h["xyz"], np.float64))
                    if amask[r, slot] != 0 and dist <= d0 + 0.5:
                        entries.append((dist - d0, anchor_entry(protein, r, atom, h["xyz"], kind="metal", metal=h["element"],
                                                                label=f"{chain_id[r]}:{int(number[r])}:{atom}={h['chain']}:{h['resseq']}:{h['name']}")))
        # a row carries at most four anchors (a carboxylate next to a metal cluster can find more): the four nearest their ideal
        # distance stay, in the order they were found, and the others are named in one warning
        keep = set()
        for r in {e[0] for _, e in entries}:
            mine = sorted((i for i, (_, e) in enumerate(entries) if e[0] == r), key=lambda i: (abs(entries[i][0]), i))
            keep.update(mine[:rc.PP_ANCHOR_PER_ROW])
        dropped = [e[5] for i, (_, e) in enumerate(entries) if i not in keep]
        if dropped:
            warn(f"anchor_sites: geometry finds more than {rc.PP_ANCHOR_PER_ROW} donor-metal contacts on a residue of {pdb_file}; "
                 f"the four nearest their ideal distance are kept, dropped: {', '.join(dropped)}")
        return anchor_set_of([e for i, (_, e) in enumerate(entries) if i in keep])
    skipped_pp = skipped_sym = 0
    for rec in link_records(pdb_file):
        ends = []
        for k in ("1", "2"):
            rows = np.nonzero((chain_id == rec["chain" + k]) & (number == rec["resseq" + k]))[0]
            std = rc.resname_to_idx.get("MET" if rec["resname" + k] == "MSE" else rec["resname" + k], 20) != 20
            ends.append((k, rows, std))
        prot = [e for e in ends if e[2] and len(e[1]) == 1]
        if len(prot) == 2:
            skipped_pp += 1
            continue
        if len(prot) != 1:
            continue
        if any(rec["sym" + k] not in ("", "1555") for k in ("1", "2")):
            skipped_sym += 1
            continue
        k, rows, _ = prot[0]
        o = "2" if k == "1" else "1"
        row, atom = int(rows[0]), rec["name" + k]
        if rec["resname" + k] == "MSE" and atom == "SE":
            atom = "SD"
        names = rc.atom14_names[int(aa[row])]
        if atom not in names or names.index(atom) < 5:
            continue                                       # a backbone atom or CB: no chi angle moves it
        tg = [h for h in het if h["chain"] == rec["chain" + o] and h["resseq"] == rec["resseq" + o] and h["name"] == rec["name" + o]
              and h["resname"] == rec["resname" + o]]
        if not tg:
            continue                                       # the partner is not in the file (a water, a hydrogen, a missing atom)
        el = tg[0]["element"]
        label = f"{chain_id[row]}:{int(number[row])}:{atom}={tg[0]['chain']}:{tg[0]['resseq']}:{tg[0]['name']}"
        if el in rc.metal_elements:
            entries.append(anchor_entry(protein, row, atom, tg[0]["xyz"], kind="metal", metal=el, label=label))
        elif el in rc.covalent_radius and atom[0] in rc.covalent_radius:
            d0 = rec["length"] if rec["length"] is not None and 1.2 <= rec["length"] <= 2.0 else rc.covalent_radius[el] + rc.covalent_radius[atom[0]]
            entries.append(anchor_entry(protein, row, atom, tg[0]["xyz"], d0=d0, kind="link", label=label))
    if skipped_pp:
        warn(f"anchor_sites: {skipped_pp} LINK record(s) between two protein residues in {pdb_file} skipped: anchors hold a fixed target")
    if skipped_sym:
        warn(f"anchor_sites: {skipped_sym} LINK record(s) to a symmetry mate in {pdb_file} skipped")
    return anchor_set_of(entries)


def link_lines(prot: Dict, anchor_set, hetero, lengths=None, keep=None) -> str:
    """The LINK records of the anchors of ``anchor_set`` (rows of ``prot``; ``keep``: the indices to write, default all) to the
    atoms of ``hetero`` (``hetero_atoms``) their targets are, 80 columns each, symmetry 1555 on both sides, the distance from
    ``lengths`` if given: the text that goes in front of ``to_pdb(prot)``, as ``ssbond_records`` does."""
    out = []
    for n, i in enumerate(range(len(anchor_set)) if keep is None else keep):
        row, slot = int(anchor_set.rows[i]), int(anchor_set.slots[i])
        tg = [h for h in hetero if np.allclose(h["xyz"], anchor_set.targets[i], atol=1e-3)]
        if not tg:
            raise ValueError(f"link_lines: no hetero atom at the target of anchor {anchor_set.labels[i] or i}")
        h = tg[0]
        rt = int(np.asarray(prot["aaindex"])[row])

        def name4(a):
            return a if len(a) == 4 else f" {a}".ljust(4)

        ln = (f"LINK        {name4(rc.atom14_names[rt][slot])} {rc.resnames[rt]:>3} {str(prot['chain_id'][row])[:1]}"
              f"{int(prot['residue_index'][row]):>4d} ").ljust(42)
        hn = h["name"]
        hname = hn.ljust(4) if (len(hn) == 4 or len(h["element"]) == 2) else f" {hn}".ljust(4)
        ln += f"{hname} {h['resname']:>3} {h['chain']}{h['resseq']:>4d}{h['icode']}".ljust(17)
        ln += f"{1555:>6d} {1555:>6d}"
        if lengths is not None:
            ln += f" {float(lengths[n]):5.2f}"
        out.append(ln.ljust(80) + "\n")
    return "".join(out)


def contains_sidechains(pdb_file) -> bool:
    """eval_diffusion.py:43-50."""
    with open(pdb_file, "r") as fh:
        for ln in fh:
            if ln.startswith("ATOM") and ln[12:16].strip() in rc.sidechain_atoms:
                return True
    return False


def _ter(serial, resname, chain, resnum) -> str:
    return f"{'TER':<6}{serial:>5}      {resname:>3} {chain:>1}{resnum:>4}"


def to_pdb(prot: Dict, keep_chains: Optional[list] = None) -> str:
    amask, aa = np.asarray(prot["atom_mask"]), np.asarray(prot["aaindex"])
    xyz, ridx = np.asarray(prot["atom_positions"]), np.asarray(prot["residue_index"])
    chain, bfac = np.asarray(prot["chain_id"]), np.asarray(prot["b_factors"])
    if np.any(aa > 20):
        raise ValueError("Invalid aaindexs.")
    if keep_chains is not None:
        sel = np.isin(chain, keep_chains)
        amask, aa, xyz, ridx, chain, bfac = amask[sel], aa[sel], xyz[sel], ridx[sel], chain[sel], bfac[sel]
    if xyz.shape[-2] != 14:
        raise ValueError("Invalid number of atoms per residue.")

    out = ["MODEL     1"]
    serial = 1
    prev_chain = chain[0]
    for i in range(aa.shape[0]):
        if chain[i] != prev_chain:
            out.append(_ter(serial, rc.resnames[aa[i - 1]], chain[i - 1], ridx[i - 1]))
            prev_chain = chain[i]
            serial += 1
        rname = rc.resnames[aa[i]]
        for aname, p, m, b in zip(rc.atom14_names[aa[i]], xyz[i], amask[i], bfac[i]):
            if m < 0.5:
                continue
            shown = aname if len(aname) == 4 else f" {aname}"
            coords = f"{p[0]:>8.3f}{p[1]:>8.3f}{p[2]:>8.3f}"
            if len(coords) != 24:
                # -1000 and below, 10000 and above: nine characters would push every column behind them one to the right
                raise ValueError(f"to_pdb: coordinate {tuple(float(v) for v in p)} of {rname} {chain[i]}{ridx[i]} {aname} does not fit "
                                 "the 8.3f columns of an ATOM record (-999.999 .. 9999.999); move the structure nearer the origin")
            out.append(f"{'ATOM':<6}{serial:>5} {shown:<4}{'':>1}{rname:>3} {chain[i]:>1}"
                       f"{ridx[i]:>4}{'':>1}   {coords}"
                       f"{1.0:>6.2f}{b:>6.2f}          {aname[0]:>2}{'':>2}")
            serial += 1
    out.append(_ter(serial, rc.resnames[aa[-1]], chain[-1], ridx[-1]))
    out += ["ENDMDL", "END"]
    return "\n".join(ln.ljust(80) for ln in out) + "\n"


def to_pdb_hydrogens(prot: Dict, hxyz, hmask) -> str:
    """``to_pdb(prot)`` with the placed hydrogens (``Context.hydrogens``: ``hxyz`` [n, 13, 3], ``hmask`` [n, 13])
    behind each residue's heavy atoms: the same records, the hydrogens named as in PDB v3 (``constants.hydrogen_names``) with
    element H and the B factor of their parent, serial numbers renumbered.  A hydrogen of an absent parent is not written."""
    amask, aa = np.asarray(prot["atom_mask"]), np.asarray(prot["aaindex"])
    xyz, ridx = np.asarray(prot["atom_positions"]), np.asarray(prot["residue_index"])
    chain, bfac = np.asarray(prot["chain_id"]), np.asarray(prot["b_factors"])
    hxyz, hmask = np.asarray(hxyz, dtype=np.float64).reshape(-1, rc.PP_H_MAX, 3), np.asarray(hmask).reshape(-1, rc.PP_H_MAX)
    if np.any(aa > 20):
        raise ValueError("Invalid aaindexs.")
    if len(hxyz) < len(aa):
        raise ValueError(f"to_pdb_hydrogens: hydrogens of {len(hxyz)} rows for {len(aa)} residues")

    def record(serial, aname, rname, i, p, b, element):
        shown = aname if len(aname) == 4 else f" {aname}"
        coords = f"{p[0]:>8.3f}{p[1]:>8.3f}{p[2]:>8.3f}"
        if len(coords) != 24:
            raise ValueError(f"to_pdb_hydrogens: coordinate {tuple(float(v) for v in p)} of {rname} {chain[i]}{ridx[i]} {aname} does not "
                             "fit the 8.3f columns of an ATOM record (-999.999 .. 9999.999); move the structure nearer the origin")
        return (f"{'ATOM':<6}{serial:>5} {shown:<4}{'':>1}{rname:>3} {chain[i]:>1}{ridx[i]:>4}{'':>1}   {coords}"
                f"{1.0:>6.2f}{b:>6.2f}          {element:>2}{'':>2}")

    out = ["MODEL     1"]
    serial = 1
    prev_chain = chain[0]
    for i in range(aa.shape[0]):
        if chain[i] != prev_chain:
            out.append(_ter(serial, rc.resnames[aa[i - 1]], chain[i - 1], ridx[i - 1]))
            prev_chain = chain[i]
            serial += 1
        rname = rc.resnames[aa[i]]
        for aname, p, m, b in zip(rc.atom14_names[aa[i]], xyz[i], amask[i], bfac[i]):
            if m < 0.5:
                continue
            out.append(record(serial, aname, rname, i, p, b, aname[0]))
            serial += 1
        for k, hname in enumerate(rc.hydrogen_names[aa[i]]):
            parent = int(rc.hydrogen_parent[aa[i], k])
            if hmask[i, k] == 0 or amask[i, parent] < 0.5:
                continue
            out.append(record(serial, hname, rname, i, hxyz[i, k], bfac[i, parent], "H"))
            serial += 1
    out.append(_ter(serial, rc.resnames[aa[-1]], chain[-1], ridx[-1]))
    out += ["ENDMDL", "END"]
    return "\n".join(ln.ljust(80) for ln in out) + "\n"
