"""Residue selections for partial repacking (``TDiffusionModule.sampling(fixed_mask=...)``, ``eval_diffusion --repack``).

A selection names the residues to REPACK; the rows outside it are the ones the sampler keeps (``fixed_mask = ~selection``).
Residues are addressed as ``featurize.mutant_data`` looks mutations up: by chain ID and the residue number of the PDB file
(``protein["chain_id"]``, ``protein["residue_index"]``) -- not by the offset numbering the featurisation gives later chains.

A selection can also be made on the device, from the batch itself: ``Context.shell(seeds, radius, mode, other_chain)``
(pp_ctx_shell) returns the rows near the ``seeds`` rows as a bool [B, L] tensor, and ``~shell`` is the
``fixed_mask`` of the partial sampler without a read-back.  ``ctx.shell(torch.ones(B, L), radius, mode="atom", other_chain=True)``
is the device interface selection: every row with an atom within ``radius`` of an atom of another chain of its complex.
``interface_selection`` below is left as it is: it reads the PDB file, so it also sees HETATM records the batch does not carry.
"""
from typing import Dict

import numpy as np


def parse_selection(spec: str, protein: Dict) -> np.ndarray:
    """Row mask [L] (bool) over ``protein`` of the residues named by ``spec``: comma-separated terms ``CHAIN`` (the whole
    chain), ``CHAIN:N`` (one residue) or ``CHAIN:N-M`` (an inclusive range; negative numbers as in ``A:-3-5``).  Insertion codes
    are not part of the protein dict: every row carrying the number is selected.  An unknown chain, a malformed term or a term
    that matches no residue raises ``ValueError``."""
    chain_id = np.asarray(protein["chain_id"])
    number = np.asarray(protein["residue_index"]).astype(np.int64)
    mask = np.zeros(len(number), dtype=bool)
    terms = [t.strip() for t in str(spec).split(",") if t.strip()]
    if not terms:
        raise ValueError("empty selection")
    for term in terms:
        chain, sep, rng = term.partition(":")
        if chain not in chain_id:
            raise ValueError(f"selection '{term}': no chain '{chain}' (chains: {', '.join(sorted(set(chain_id.tolist())))})")
        rows = chain_id == chain
        if sep:
            try:
                cut = rng.find("-", 1)          # a leading '-' is a sign
                lo, hi = (int(rng), int(rng)) if cut < 0 else (int(rng[:cut]), int(rng[cut + 1:]))
            except ValueError:
                raise ValueError(f"selection '{term}': expected CHAIN, CHAIN:N or CHAIN:N-M") from None
            rows = rows & (number >= lo) & (number <= hi)
        if not rows.any():
            raise ValueError(f"selection '{term}' matches no residue")
        mask |= rows
    return mask


def residue_names(protein: Dict):
    """[(chain ID, PDB residue number)] per row of ``protein``: what ``batch.residue_names`` holds for
    ``TDiffusionModule.sampling(disulfides=SPEC)``."""
    return [(str(c), int(n)) for c, n in zip(protein["chain_id"], protein["residue_index"])]


def parse_disulfides(spec, protein: Dict):
    """Row pairs [(a, b)] of the residue pairs named by ``spec``: a string of comma-separated terms ``CHAIN:N-CHAIN:M`` (chain ID and
    PDB residue number, negative numbers as in ``A:-3-A:12``) or a list of ``((chain, number), (chain, number))``.  ``ValueError``
    for a malformed term, a residue that does not exist (unknown chain or number) and a number that several rows carry (insertion
    codes are not part of the protein dict).  Whether the rows are cysteines that can bond is checked where the batch is
    (``lib.Context.check_disulfide_pairs``)."""
    import re
    chain_id = np.asarray(protein["chain_id"])
    number = np.asarray(protein["residue_index"]).astype(np.int64)
    if isinstance(spec, str):
        terms = [t.strip() for t in spec.split(",") if t.strip()]
        if not terms:
            raise ValueError("empty disulfide list")
        named = []
        for term in terms:
            m = re.fullmatch(r"([^:\s]+):(-?\d+)-([^:\s]+):(-?\d+)", term)
            if m is None:
                raise ValueError(f"disulfides '{term}': expected CHAIN:N-CHAIN:M")
            named.append(((m.group(1), int(m.group(2))), (m.group(3), int(m.group(4)))))
    else:
        try:
            named = [((str(a[0]), int(a[1])), (str(b[0]), int(b[1]))) for a, b in spec]
        except (TypeError, ValueError, IndexError):
            raise ValueError("disulfides: expected a list of ((chain, number), (chain, number))") from None
    pairs = []
    for ends in named:
        rows = []
        for chain, num in ends:
            hit = np.nonzero((chain_id == chain) & (number == num))[0]
            if len(hit) == 0:
                raise ValueError(f"disulfides: no residue {chain}:{num}")
            if len(hit) > 1:
                raise ValueError(f"disulfides: {len(hit)} rows carry {chain}:{num}")
            rows.append(int(hit[0]))
        pairs.append((rows[0], rows[1]))
    return pairs


class AnchorSet:
    """The anchors of one complex (pp_anchor_close): ``rows``, ``slots``, ``antes`` int32 [A] (the row, the
    donor's atom14 slot, the slot the donor is bonded to), ``targets`` float32 [A, 3] (the fixed points, in the coordinates of the
    batch), ``params`` float32 [A, 4] (d0, sigma_d, theta0, sigma_theta; sigma_theta <= 0: no angle term), ``labels`` (one text per
    anchor, what a refusal names) and ``kinds`` ("metal", "link" or "").  Rows count from the first row of the complex; ``shifted``
    moves them to the rows of a packed batch and records the ``segment`` they must then lie in (None claims nothing)."""

    def __init__(self, rows=(), slots=(), antes=(), targets=(), params=(), labels=None, kinds=None, segment=None):
        self.rows = np.asarray(rows, np.int32).reshape(-1)
        A = len(self.rows)
        self.slots = np.asarray(slots, np.int32).reshape(-1)
        self.antes = np.asarray(antes, np.int32).reshape(-1)
        self.targets = np.asarray(targets, np.float32).reshape(-1, 3)
        self.params = np.asarray(params, np.float32).reshape(-1, 4)
        self.labels = [str(x) for x in labels] if labels is not None else [""] * A
        self.kinds = [str(x) for x in kinds] if kinds is not None else [""] * A
        self.segment = segment
        for name, v in (("slots", self.slots), ("antes", self.antes), ("targets", self.targets), ("params", self.params),
                        ("labels", self.labels), ("kinds", self.kinds)):
            if len(v) != A:
                raise ValueError(f"AnchorSet: {len(v)} {name} for {A} rows")

    def __len__(self):
        return len(self.rows)

    def shifted(self, offset: int, segment=None):
        return AnchorSet(self.rows + int(offset), self.slots, self.antes, self.targets, self.params, self.labels, self.kinds, segment)

    def subset(self, keep):
        """The anchors with the indices ``keep``, in that order; the segment claim stays."""
        keep = [int(i) for i in keep]
        return AnchorSet(self.rows[keep], self.slots[keep], self.antes[keep], self.targets[keep], self.params[keep],
                         [self.labels[i] for i in keep], [self.kinds[i] for i in keep], self.segment)

    @staticmethod
    def concat(sets):
        """One set of the anchors of ``sets`` in their order; it claims no segment (each part was checked against its own)."""
        sets = list(sets)
        if not sets:
            return AnchorSet()
        return AnchorSet(np.concatenate([s.rows for s in sets]), np.concatenate([s.slots for s in sets]),
                         np.concatenate([s.antes for s in sets]), np.concatenate([s.targets for s in sets]),
                         np.concatenate([s.params for s in sets]), sum((s.labels for s in sets), []), sum((s.kinds for s in sets), []))

    def device_arrays(self, device):
        """(int32 [A, 4] (row, slot, ante, 0), float32 [A, 4] target, float32 [A, 4] params) on ``device``, as pp_anchor_close reads
        them; one row of zeros for an empty set (the call is given A = 0)."""
        import torch
        A = max(len(self), 1)
        ai, at, ap = np.zeros((A, 4), np.int32), np.zeros((A, 4), np.float32), np.zeros((A, 4), np.float32)
        if len(self):
            ai[:, 0], ai[:, 1], ai[:, 2] = self.rows, self.slots, self.antes
            at[:, :3] = self.targets
            ap[:] = self.params
        return tuple(torch.from_numpy(x).to(device).contiguous() for x in (ai, at, ap))


def check_anchor_set(anchor_set, rt, rm, am, seg_offsets, names=None):
    """Refuse, by name, what pp_anchor_close would drop (the rules of csrc/pp_anchor.hip restated on host arrays: ``rt`` [N] residue
    types, ``rm`` [N] residue mask, ``am`` [N, 14] atom mask, ``seg_offsets`` the segment table) and an anchor outside the segment
    the set claims.  ``lib.Context.check_anchors`` calls it with the context's own arrays."""
    from bisect import bisect_right
    from . import constants as rc
    A, n_rows = len(anchor_set), len(rt)
    a2g = np.asarray(rc.atom14_to_group)
    offs, per_row = list(seg_offsets), {}
    for i in range(A):
        r, slot, ante = int(anchor_set.rows[i]), int(anchor_set.slots[i]), int(anchor_set.antes[i])
        what = f"anchor {anchor_set.labels[i]}" if anchor_set.labels[i] else f"anchor {i}"
        if not 0 <= r < n_rows:
            raise ValueError(f"anchors: {what}: row {r} is outside the {n_rows} rows of this context")
        where = str(names[r]) if names is not None else f"row {r}"
        if anchor_set.segment is not None and bisect_right(offs, r) - 1 != int(anchor_set.segment):
            raise ValueError(f"anchors: {what}: {where} lies in segment {bisect_right(offs, r) - 1}, the set claims segment "
                             f"{int(anchor_set.segment)}")
        if not 0 <= int(rt[r]) <= 20 or rm[r] == 0:
            raise ValueError(f"anchors: {what}: {where} is masked out")
        if not 5 <= slot <= 13 or not 4 <= int(a2g[int(rt[r]), slot]) <= 7:
            raise ValueError(f"anchors: {what}: slot {slot} of {where} is no side-chain atom that a chi angle moves")
        if not 0 <= ante <= 13 or ante == slot:
            raise ValueError(f"anchors: {what}: antecedent slot {ante} of {where} must be another slot 0..13 of the row")
        for sl in (0, 1, 2, slot, ante):
            if am[r, sl] == 0:
                raise ValueError(f"anchors: {what}: {where} lacks {rc.atom14_names[int(rt[r])][sl] or 'slot ' + str(sl)}")
        vals = np.concatenate([np.asarray(anchor_set.targets[i], np.float32), np.asarray(anchor_set.params[i], np.float32)])
        if not np.isfinite(vals).all() or not vals[4] > 0:
            raise ValueError(f"anchors: {what}: target, d0, sigma_d, theta0 and sigma_theta must be finite and sigma_d positive")
        per_row[r] = per_row.get(r, 0) + 1
        if per_row[r] > 4:
            raise ValueError(f"anchors: {what}: the fifth anchor on {where} (a row carries at most 4)")
    return anchor_set


def anchor_entry(protein: Dict, row: int, atom: str, target, d0=None, kind="metal", metal=None, label=None):
    """(row, slot, ante, target, (d0, sigma_d, theta0, sigma_theta), label, kind) of one anchor of ``protein``: the donor ``atom`` of
    ``row`` by name, its antecedent from the covalent bonds (``constants.anchor_antecedent``), the angle term from
    ``constants.anchor_angle`` (none for a donor it does not list), ``d0`` from ``constants.metal_distance`` if not given."""
    from . import constants as rc
    rt = int(np.asarray(protein["aaindex"])[row])
    names = rc.atom14_names[rt]
    where = f"{str(protein['chain_id'][row])}:{int(protein['residue_index'][row])}"
    if atom not in names or names.index(atom) < 5:
        raise ValueError(f"anchors: {rc.resnames[rt]} {where} has no side-chain atom {atom} beyond CB")
    slot = names.index(atom)
    th0, st = rc.anchor_angle.get(rc.resnames[rt], {}).get(atom, (0.0, 0.0))
    if d0 is None:
        if metal is None:
            raise ValueError(f"anchors: {where}:{atom} needs d0 or a metal")
        d0 = rc.metal_distance(metal, atom[0])
    sd = rc.ANCHOR_SIGMA_D_METAL if kind == "metal" else rc.ANCHOR_SIGMA_D_COVALENT
    return (int(row), slot, rc.anchor_antecedent(rt, slot), np.asarray(target, np.float32).reshape(3), (float(d0), sd, th0, st),
            label or f"{where}:{atom}", kind)


def anchor_set_of(entries, segment=None) -> "AnchorSet":
    entries = list(entries)
    return AnchorSet(*[[e[k] for e in entries] for k in range(7)], segment=segment)


def parse_anchors(spec, protein: Dict, hetero) -> "AnchorSet":
    """The ``AnchorSet`` named by ``spec``: comma-separated terms ``CHAIN:N:ATOM=CHAIN:N:ATOM`` -- left a side-chain atom of a
    residue of ``protein`` (chain ID, PDB residue number, atom name), right an atom of ``hetero`` (``pdb_io.hetero_atoms``: the
    HETATM and non-standard-residue atoms of the file).  A metal target gives the metal's distance and sigma_d, any other target a
    covalent link (the sum of the covalent radii).  ``ValueError`` for a malformed term, a residue or atom that does not exist, a
    number that several rows carry, a target that several atoms match."""
    import re
    from . import constants as rc
    chain_id = np.asarray(protein["chain_id"])
    number = np.asarray(protein["residue_index"]).astype(np.int64)
    terms = [t.strip() for t in str(spec).split(",") if t.strip()]
    if not terms:
        raise ValueError("empty anchor list")
    entries = []
    for term in terms:
        m = re.fullmatch(r"([^:\s]+):(-?\d+):([^:=\s]+)=([^:\s]+):(-?\d+):([^:=\s]+)", term)
        if m is None:
            raise ValueError(f"anchors '{term}': expected CHAIN:N:ATOM=CHAIN:N:ATOM")
        chain, num, atom, tchain, tnum, tatom = m.group(1), int(m.group(2)), m.group(3), m.group(4), int(m.group(5)), m.group(6)
        hit = np.nonzero((chain_id == chain) & (number == num))[0]
        if len(hit) == 0:
            raise ValueError(f"anchors: no residue {chain}:{num}")
        if len(hit) > 1:
            raise ValueError(f"anchors: {len(hit)} rows carry {chain}:{num}")
        tg = [h for h in hetero if h["chain"] == tchain and h["resseq"] == tnum and h["name"] == tatom]
        if len(tg) != 1:
            raise ValueError(f"anchors: {len(tg)} hetero atoms match {tchain}:{tnum}:{tatom}")
        el = tg[0]["element"]
        if el in rc.metal_elements:
            entries.append(anchor_entry(protein, int(hit[0]), atom, tg[0]["xyz"], kind="metal", metal=el, label=term))
        else:
            if el not in rc.covalent_radius or atom[0] not in rc.covalent_radius:
                raise ValueError(f"anchors '{term}': no covalent radius for {el} or {atom[0]}")
            entries.append(anchor_entry(protein, int(hit[0]), atom, tg[0]["xyz"], d0=rc.covalent_radius[el] + rc.covalent_radius[atom[0]],
                                        kind="link", label=term))
    return anchor_set_of(entries)


DEVICE_SELECTORS = {"interface:sasa": "interface", "pocket": "pocket"}       # --repack words answered by Context.sasa


def device_selector(spec, obstacles: str = "none"):
    """"interface" / "pocket" if ``spec`` is one of the ``--repack`` words that ``sasa_selection`` answers ("interface:sasa",
    "pocket"), else None (a residue list, or the file-based "interface").  ``obstacles``: the command line's ``--obstacles``
    mode; "pocket" selects the rows whose surface the obstacle atoms bury, so without any it is refused (``ValueError``)."""
    kind = DEVICE_SELECTORS.get(str(spec).strip()) if spec is not None else None
    if kind == "pocket" and obstacles in (None, "none"):
        raise ValueError("--repack pocket selects the residues whose surface the obstacle atoms bury: it needs --obstacles "
                         "hetero or hetero+water")
    return kind


def sasa_selection(batch, kind: str, n_points: int = 96, probe: float = 1.4) -> np.ndarray:
    """Row mask [L] (bool) of a B = 1 batch on the device, made there from the batch's own coordinates (``Context.sasa``, DESIGN.md
    section 20; no PDB re-read): ``kind`` "interface" = the delta-SASA interface, rows with a test point that is exposed in the
    isolated chain and buried in the complex (the rule of the reference's interface.py, which needs freesasa); "pocket" = rows
    with a test point that only the batch's obstacle atoms bury.  ``ValueError`` if no row qualifies."""
    from .functional import solvent_accessibility
    if kind not in ("interface", "pocket"):
        raise ValueError(f"kind must be 'interface' or 'pocket', got {kind!r}")
    res = solvent_accessibility(batch, n_points=n_points, probe=probe)
    mask = (res.interface if kind == "interface" else res.pocket)[0].cpu().numpy().astype(bool)
    if not mask.any():
        raise ValueError("no residue buries surface against another chain" if kind == "interface" else
                         "no residue's surface is buried by an obstacle atom")
    return mask


def interface_selection(protein: Dict, pdb, radius: float = 10.0) -> np.ndarray:
    """Row mask [L] (bool) of the interface: residues with an atom within ``radius`` of another protein chain
    (``analysis.interface_residues`` on the file, matched by chain ID and file numbering).  ``ValueError`` if the file has fewer
    than two protein chains or no residue qualifies."""
    from .analysis import interface_residues
    inter = interface_residues(pdb, radius)
    if inter is None:
        raise ValueError(f"{pdb}: an interface needs at least two protein chains")
    chain_id = np.asarray(protein["chain_id"])
    number = np.asarray(protein["residue_index"]).astype(np.int64)
    mask = np.zeros(len(number), dtype=bool)
    for chain, numbers in inter.items():
        mask |= (chain_id == chain) & np.isin(number, numbers)
    if not mask.any():
        raise ValueError(f"{pdb}: no residue within {radius} A of another chain")
    return mask
