"""The ``batch`` object the sampler consumes.

The reference uses a ``torch_geometric.data.Data`` filled by ``prot_to_data``
(complex_dataset.py:123-139) and padded/stacked by ``collate_fn``
(complex_datamodule.py:196-226).  This is a dependency-free container with the same
attribute / item access and ``.to(device)``.
"""
from typing import Iterable, List

import torch
import torch.nn.functional as F

TENSOR_KEYS = (
    "X", "atom_mask", "residue_type", "residue_mask", "residue_index", "chain_indices",
    "BB_D", "BB_D_sincos", "BB_D_mask", "SC_D", "SC_D_sincos", "SC_D_mask",
    "chi_1pi_periodic_mask", "chi_2pi_periodic_mask",
)
# The extra per-residue keys of a PackPPI-AP batch (skempi_dataset.py:220-252): the mutation mask and the mutant's copies of
# the wild-type keys that AffinityPrediction.forward swaps in (AffinityPrediction.py:178-181).
MUT_KEYS = (
    "mut_mask", "atom_mask_mut", "residue_type_mut", "SC_D_mut", "SC_D_sincos_mut", "SC_D_mask_mut",
    "chi_1pi_periodic_mask_mut", "chi_2pi_periodic_mask_mut",
)
# every per-residue key skempi_datamodule.collate_fn stacks (skempi_datamodule.py:245-287), in its order
AFFINITY_KEYS = (
    "mut_mask", "X", "residue_mask", "residue_index", "chain_indices", "BB_D", "BB_D_sincos", "BB_D_mask",
    "atom_mask", "residue_type", "SC_D", "SC_D_sincos", "SC_D_mask", "chi_1pi_periodic_mask", "chi_2pi_periodic_mask",
    "atom_mask_mut", "residue_type_mut", "SC_D_mut", "SC_D_sincos_mut", "SC_D_mask_mut", "chi_1pi_periodic_mask_mut",
    "chi_2pi_periodic_mask_mut",
)


# optional per-residue keys that pack() carries when every complex has them: the rows partial repacking keeps
# (``TDiffusionModule.sampling(fixed_mask=...)``; [L] or [1, L], 1 = keep)
ROW_KEYS = ("fixed_mask",)


# obstacle atoms (``featurize.protein_to_batch(..., obstacles=...)``): ``obstacle_xyzr`` [M, 4] float32
# (x, y, z, radius) and ``obstacle_offsets`` int32 [n + 1] -- complex (or, in a batch of decoys, group) k owns the atoms
# obstacle_offsets[k] .. obstacle_offsets[k + 1] - 1 --, with ``obstacle_offsets_host``, the same as a list.  Not per-residue
# tensors: nothing gives them a batch axis, pads or slices them.  A batch without obstacles has none of the keys.
# ``obstacle_polar`` uint8 [M] (1 = a polar atom, N or O: what ``Context.polar`` counts as a partner) rides
# along where the obstacles came with their elements (``pdb_io.obstacle_atoms``); a batch whose obstacles have none lacks the key.
OBSTACLE_KEYS = ("obstacle_xyzr", "obstacle_offsets", "obstacle_offsets_host", "obstacle_polar")


def has_obstacles(b) -> bool:
    return hasattr(b, "get") and b.get("obstacle_xyzr") is not None


def _obstacles_of(c):
    """(xyzr [M, 4], M) of one complex (per-complex data or a B = 1 batch); (None, 0) without obstacles."""
    if not has_obstacles(c):
        return None, 0
    offs = c.get("obstacle_offsets_host") or [int(x) for x in c["obstacle_offsets"].tolist()]
    if len(offs) != 2:
        raise ValueError(f"a single complex carries one obstacle range, this one has {len(offs) - 1}")
    x = c["obstacle_xyzr"].reshape(-1, 4)
    return x[offs[0]:offs[1]], offs[1] - offs[0]


def _obstacle_polar_of(c):
    """uint8 [M] of one complex: its ``obstacle_polar`` cut to its range, or None (no obstacles, or obstacles without the key)."""
    if not has_obstacles(c) or c.get("obstacle_polar") is None:
        return None
    offs = c.get("obstacle_offsets_host") or [int(x) for x in c["obstacle_offsets"].tolist()]
    return c["obstacle_polar"].reshape(-1)[offs[0]:offs[1]]


def _set_obstacles(out, parts, like, polar=None):
    """Store the obstacle keys of a batch whose complexes (groups) own the atom blocks ``parts`` ([M_k, 4] or None), in order.
    ``polar``: the complexes' ``obstacle_polar`` blocks (or None each); if any complex has one the batch gets the key, with zeros
    for the atoms of a complex that has none."""
    if polar is not None and any(q is not None for q in polar):
        blocks = [(q.to(device=like.device, dtype=torch.uint8) if q is not None else
                   torch.zeros(int(p.shape[0]), dtype=torch.uint8, device=like.device)) for p, q in zip(parts, polar) if p is not None]
        out["obstacle_polar"] = torch.cat(blocks, 0) if blocks else torch.zeros(0, dtype=torch.uint8, device=like.device)
    offs = [0]
    for p in parts:
        offs.append(offs[-1] + (0 if p is None else int(p.shape[0])))
    blocks = [p.to(device=like.device, dtype=torch.float32) for p in parts if p is not None]
    out["obstacle_xyzr"] = torch.cat(blocks, 0) if blocks else torch.zeros(0, 4, device=like.device)
    out["obstacle_offsets"] = torch.tensor(offs, dtype=torch.int32).to(like.device, non_blocking=True)
    out["obstacle_offsets_host"] = offs


class Batch(dict):
    """Attribute-style dict: ``batch.X``, ``batch['X']``, ``batch.to('cuda')``, ``batch.keys()``."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e

    def __setattr__(self, k, v):
        self[k] = v

    def to(self, device):
        out = Batch()
        for k, v in self.items():
            out[k] = v.to(device) if isinstance(v, torch.Tensor) else v
        return out

    def clone(self):
        out = Batch()
        for k, v in self.items():
            out[k] = v.clone() if isinstance(v, torch.Tensor) else v
        return out

    def apply(self, fn):
        for k in list(self.keys()):
            self[k] = fn(self[k])
        return self

    def true_residues(self) -> int:
        return int(self["residue_mask"].sum().item())


def as_single(data: Batch) -> Batch:
    """Add the leading batch axis the way ``ProteinAnalysis.get_prot`` does (protein_analysis.py:115-120)."""
    out = Batch()
    for k, v in data.items():
        out[k] = v.unsqueeze(0) if isinstance(v, torch.Tensor) and k not in OBSTACLE_KEYS else v
    out["num_proteins"] = 1
    out["max_size"] = int(data["num_nodes"])
    return out


def collate(proteins: Iterable[Batch]) -> Batch:
    """Pad every per-residue tensor to the longest complex and stack (complex_datamodule.py:196-226).  Obstacle atoms are not
    supported in padded batches (``ValueError``): use ``pack``."""
    proteins = list(proteins)
    if any(has_obstacles(p) for p in proteins):
        raise ValueError("collate: a padded batch cannot carry obstacle atoms; use batch.pack()")
    max_size = max(int(p["num_nodes"]) for p in proteins)

    def pad(p, key):
        t = p[key]
        return F.pad(t, [0, 0] * (t.dim() - 1) + [0, max_size - int(p["num_nodes"])])

    out = Batch(num_proteins=len(proteins), max_size=max_size)
    for key in TENSOR_KEYS:
        out[key] = torch.stack([pad(p, key) for p in proteins])
    return out


def collate_affinity(proteins: Iterable[Batch]) -> Batch:
    """Padded batch of ``featurize.mutant_data`` outputs: ``ddg`` [B] plus every per-residue key padded with zeros to the
    longest complex and stacked (skempi_datamodule.py:245-287)."""
    proteins = list(proteins)
    max_size = max(int(p["num_nodes"]) for p in proteins)

    def pad(p, key):
        t = p[key]
        return F.pad(t, [0, 0] * (t.dim() - 1) + [0, max_size - int(p["num_nodes"])])

    out = Batch(num_proteins=len(proteins), max_size=max_size, ddg=torch.stack([p["ddg"] for p in proteins]))
    for key in AFFINITY_KEYS:
        out[key] = torch.stack([pad(p, key) for p in proteins])
    return out


def split(batch: Batch) -> List[Batch]:
    """Inverse of ``collate`` up to padding: one B=1 batch per complex (padding kept)."""
    outs = []
    for b in range(int(batch["num_proteins"])):
        o = Batch(num_proteins=1, max_size=int(batch["max_size"]))
        for k in TENSOR_KEYS:
            o[k] = batch[k][b:b + 1]
        if has_obstacles(batch):          # only a B = 1 batch can have them (collate refuses): its one complex keeps them
            for k in OBSTACLE_KEYS:
                if k in batch:
                    o[k] = batch[k]
        outs.append(o)
    return outs


def pack(complexes: Iterable[Batch], trim: bool = True) -> Batch:
    """Ragged batch WITHOUT padding rows: the complexes' rows back to back in one [1, sum of lengths, ...] batch, plus
    ``seg_offsets`` (int32 [n + 1]: first row of every complex, then the total; ``seg_offsets_host`` is the same as a list,
    so that nothing has to be read back from the device).

    The reference pads to the longest complex and stacks (``collate``; complex_datamodule.py:196-226) and then computes on
    the padding rows as well; the path has no cross-complex term, so a packed batch gives every complex the result of
    running it alone (``lib.Context`` / ``pp_complex_prepare_packed``).  Accepts per-complex data (``protein_to_data``,
    tensors [L, ...]) or B = 1 batches ([1, L, ...]).  Only TRAILING padding is dropped: a complex keeps its rows up to the
    last true residue, so a residue masked out in the middle of a chain (a missing backbone atom: featurize.py) stays in
    place with its ``residue_mask`` 0, exactly as the reference carries it.

    ``trim=False`` keeps every row, trailing padding included (PackPPI-AP: the max over residues of AffinityPrediction.py:186
    sees those rows).  Complexes that all carry the PackPPI-AP keys (``mut_mask``, the ``*_mut`` keys, ``ddg``) keep them:
    the per-row keys are packed like the others, ``ddg`` becomes [n].  Complexes that all carry a ``complex_key`` (an int: the
    key of the seeded sampling noise, ``TDiffusionModule.sampling(seed=...)``) give the batch ``complex_keys``, a list in packing
    order; batches without it pack as before.  Complexes that all carry a ``fixed_mask`` ([L] or [1, L]: the rows partial
    repacking keeps) give the batch its ``fixed_mask`` [1, N]; ``unpack`` splits it like any per-row result.  If any complex
    carries obstacle atoms (``OBSTACLE_KEYS``) the batch does: the blocks back to back, one range per complex (empty for a complex
    without); if none does, the batch has none of the keys."""
    complexes = list(complexes)
    keys = TENSOR_KEYS + tuple(k for k in MUT_KEYS + ROW_KEYS if all(k in c for c in complexes))
    rows = {k: [] for k in keys}
    offs = [0]
    ends = []
    for c in complexes:
        lead = c["residue_type"].dim() == 2
        if lead and c["residue_type"].shape[0] != 1:
            raise ValueError("pack() takes single complexes (use split() on a padded batch first)")
        keep = (c["residue_mask"][0] if lead else c["residue_mask"]) > 0
        # index of the last true residue + 1 (0 for an empty complex), computed where the mask lives
        ends.append((keep * torch.arange(1, keep.numel() + 1, device=keep.device)).max() if trim else
                    torch.tensor(keep.numel(), device=keep.device))
    ends = [int(x) for x in torch.stack(ends).tolist()]            # ONE read-back for the whole batch
    for c, n in zip(complexes, ends):
        if n == 0:
            raise ValueError("empty complex")
        lead = c["residue_type"].dim() == 2
        for k in keys:
            t = c[k][0] if lead else c[k]
            rows[k].append(t[:n])
        offs.append(offs[-1] + n)
    out = Batch(num_proteins=1, max_size=offs[-1])
    for k in keys:
        out[k] = torch.cat(rows[k], 0).unsqueeze(0)
    if all("ddg" in c for c in complexes):
        out["ddg"] = torch.cat([c["ddg"].reshape(-1) for c in complexes])
    if complexes and all(c.get("complex_key") is not None for c in complexes):
        out["complex_keys"] = [int(c["complex_key"]) for c in complexes]
    out["seg_offsets"] = torch.tensor(offs, dtype=torch.int32).to(out["X"].device, non_blocking=True)
    out["seg_offsets_host"] = offs
    if any(has_obstacles(c) for c in complexes):
        _set_obstacles(out, [_obstacles_of(c)[0] for c in complexes], out["X"], [_obstacle_polar_of(c) for c in complexes])
    return out


def unpack(packed: Batch, t: torch.Tensor) -> List[torch.Tensor]:
    """Split a per-row result [1, sum of lengths, ...] of a packed batch into one [1, L_i, ...] tensor per complex."""
    offs = packed.get("seg_offsets_host") or [int(x) for x in packed["seg_offsets"].tolist()]
    return [t[:, a:b] for a, b in zip(offs[:-1], offs[1:])]


def pad_rows(t: torch.Tensor, n: int, tail=0, fresh: bool = False) -> torch.Tensor:
    """A per-row result [1, m, ...] of one complex with the trailing rows ``pack`` dropped put back: [1, n, ...].  ``tail``: what
    the rows m .. n - 1 hold -- a number, or a tensor [1, n, ...] whose rows m .. n - 1 they are.  m == n: ``t`` itself, a view of
    the packed result, unless ``fresh`` asks for a tensor of its own."""
    m = t.shape[1]
    if m == n and not fresh:
        return t
    if isinstance(tail, torch.Tensor):
        return torch.cat([t, tail[:, m:]], 1)
    full = torch.full((1, n) + tuple(t.shape[2:]), tail, device=t.device, dtype=t.dtype)
    full[:, :m] = t
    return full


def group_rows(sizes, alone, max_rows, mult: int = 1) -> List[List[int]]:
    """How the drivers cut a list of complexes into packed batches: groups of indices into ``sizes`` (rows per complex), in order.
    An ``alone`` complex (shorter than 32 rows: K = min(32, L) is a property of the batch) is a group of its own, put down where it
    stands; the others fill a group while ``mult`` x its rows stays within ``max_rows`` (``mult``: rows launched per row of the
    group, the decoys of an ensemble)."""
    groups, cur, rows_in = [], [], 0
    for i, (n, solo) in enumerate(zip(sizes, alone)):
        if solo:
            groups.append([i])
            continue
        if cur and mult * (rows_in + n) > max_rows:
            groups.append(cur)
            cur, rows_in = [], 0
        cur.append(i)
        rows_in += n
    if cur:
        groups.append(cur)
    return groups


# ---- decoy ensembles ---------------------------------------------------------------------------------------
_M64 = (1 << 64) - 1


def decoy_key(key: int, d: int) -> int:
    """The 64-bit noise key of decoy ``d`` of the complex whose key is ``key`` (``TDiffusionModule.sampling(seed=...)`` keys,
    DESIGN.md section 12).  ``decoy_key(k, 0) == k``: decoy 0 is the complex as it is sampled today.  For ``d >= 1`` it is the
    SplitMix64 finaliser of ``z = (k + d * 0x9E3779B97F4A7C15) mod 2**64``::

        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9 mod 2**64
        z = (z ^ (z >> 27)) * 0x94D049BB133111EB mod 2**64
        z =  z ^ (z >> 31)

    The finaliser is a bijection of the 64-bit words, so for one ``d`` different complexes keep different keys; no bits of ``k``
    are set aside for ``d`` (keys of 2**40 and above are in use)."""
    key, d = int(key) & _M64, int(d)
    if d < 0:
        raise ValueError("decoy index must not be negative")
    if d == 0:
        return key
    z = (key + d * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _base_key(c, ordinal: int) -> int:
    """The key ``sampling(seed=...)`` would give this complex alone or at place ``ordinal`` of a batch: its ``complex_key``, a B = 1
    batch's one ``complex_keys`` entry, else the ordinal."""
    k = c.get("complex_key") if hasattr(c, "get") else None
    if k is None and hasattr(c, "get") and c.get("complex_keys") is not None:
        ks = c["complex_keys"]
        ks = ks.tolist() if isinstance(ks, torch.Tensor) else list(ks)
        if len(ks) != 1:
            raise ValueError(f"a B = 1 batch carries one complex key, this one has {len(ks)}")
        k = ks[0]
    return (int(k) if k is not None else int(ordinal)) & _M64


def replicate_many(complexes: Iterable[Batch], n_decoys: int, keys=None) -> Batch:
    """``n_decoys`` copies of every complex in one packed batch, group-major: segment ``g * n_decoys + d`` is decoy ``d`` of complex
    ``g`` and carries the key ``decoy_key(k_g, d)``, where ``k_g`` is ``keys[g]`` if given, else the complex's ``complex_key`` if it
    has one, else ``g``.  The batch gets ``complex_keys`` (what the seeded sampler reads), ``n_decoys`` and ``n_groups``.  Takes what
    ``pack`` takes: per-complex data or B = 1 batches.

    Obstacle atoms (``OBSTACLE_KEYS``) are carried per GROUP: ``obstacle_offsets`` has one range per complex, shared by its decoys.

    ``ValueError``: ``n_decoys < 1``, no complex, keys of this call that are not pairwise distinct (two segments would draw the same
    noise), or a group whose copies differ in length (impossible through this function; ``lib.Context.ensemble_reduce`` relies on it)."""
    complexes = list(complexes)
    n_decoys = int(n_decoys)
    if n_decoys < 1:
        raise ValueError(f"n_decoys must be at least 1, got {n_decoys}")
    if not complexes:
        raise ValueError("replicate_many needs at least one complex")
    if keys is not None and len(keys) != len(complexes):
        raise ValueError(f"{len(keys)} keys for {len(complexes)} complexes")
    base = [(int(keys[g]) & _M64) if keys is not None else _base_key(c, g) for g, c in enumerate(complexes)]
    all_keys = [decoy_key(k, d) for k in base for d in range(n_decoys)]
    if len(set(all_keys)) != len(all_keys):
        raise ValueError("the decoy keys of this call are not pairwise distinct: two segments would draw the same noise "
                         f"(base keys {base}, n_decoys {n_decoys})")
    # a copy must not bring a key of its own into pack(): the keys are set below
    plain = [Batch({k: v for k, v in c.items() if k not in ("complex_key", "complex_keys") + OBSTACLE_KEYS}) for c in complexes]
    out = pack([c for c in plain for _ in range(n_decoys)])
    check_groups(out["seg_offsets_host"], n_decoys)
    # obstacles belong to the group: one range per complex, which its n_decoys segments share (lib.Context maps segment s to
    # range s // n_decoys)
    if any(has_obstacles(c) for c in complexes):
        _set_obstacles(out, [_obstacles_of(c)[0] for c in complexes], out["X"], [_obstacle_polar_of(c) for c in complexes])
    out["complex_keys"] = all_keys
    out["n_decoys"] = n_decoys
    out["n_groups"] = len(complexes)
    return out


def replicate(complex_or_b1_batch: Batch, n_decoys: int, key=None) -> Batch:
    """``pack([c] * n_decoys)`` with ``complex_keys = [decoy_key(k, d) for d in range(n_decoys)]``, ``n_decoys`` and
    ``n_groups = 1``: the decoys of one complex as the segments of one packed batch.  ``k`` is ``key`` if given, else the complex's
    own key (``complex_key``, or a B = 1 batch's ``complex_keys`` entry), else 0 -- the key the complex has when it is sampled alone.
    ``ValueError`` as ``replicate_many``."""
    return replicate_many([complex_or_b1_batch], n_decoys, keys=None if key is None else [key])


def check_groups(seg_offsets: List[int], n_decoys: int) -> List[int]:
    """The group lengths of a segment table made of groups of ``n_decoys`` consecutive segments of equal length; ``ValueError`` if
    the table is not one (what ``pp_ensemble_reduce`` takes: the consensus row of (group g, row r) is
    ``seg_offsets[g * n_decoys] / n_decoys + r``)."""
    offs = [int(x) for x in seg_offsets]
    n_seg = len(offs) - 1
    if n_decoys < 1:
        raise ValueError(f"n_decoys must be at least 1, got {n_decoys}")
    if n_seg < 1 or n_seg % n_decoys:
        raise ValueError(f"{n_seg} segments are not groups of {n_decoys} decoys")
    lens = [b - a for a, b in zip(offs[:-1], offs[1:])]
    out = []
    for g in range(n_seg // n_decoys):
        grp = lens[g * n_decoys:(g + 1) * n_decoys]
        if min(grp) < 1 or len(set(grp)) != 1:
            raise ValueError(f"the {n_decoys} decoys of group {g} differ in length: {grp}")
        out.append(grp[0])
    return out
