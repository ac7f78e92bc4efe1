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
