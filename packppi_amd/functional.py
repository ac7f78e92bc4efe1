"""Free functions of the reference's hot path, same names and argument meaning, HIP-backed.

    get_atom14_coords(X, S, BB_D, SC_D)                       components/__init__.py:76-120
    compute_residue_clash(batch, SC_D, vtf=12., tol=0.5)       clash.py:335-365
    find_clash_mask(batch, SC_D, vtf, tol)                     optimize.py:5-18
    proximal_optimizer(batch, SC_D, vtf, tol, lamda, steps)    optimize.py:21-73
    proximal_optimizer_packed(packed_batch, SC_D, ...)        the same for every complex of a batch.pack() batch at once
    solvent_accessibility(batch, SC_D=None, ...)              no reference counterpart (interface.py needs freesasa): pp_sasa

The three proximal functions take ``fixed_mask`` (partial repacking): rows that keep their incoming angles.

All tensors must live on the MI355X; there is no CPU path here.
"""
from typing import List, Tuple

import torch

from .batch import Batch
from .lib import BatchKey, Context, Plan

_geometry_plans = {}


def geometry_plan(device) -> Plan:
    """Weight-free plan (chemistry tables only), one per device."""
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError(f"packppi_amd needs tensors on the HIP device, got {device}")
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _geometry_plans:
        _geometry_plans[idx] = Plan(None, torch.device("cuda", idx))
    return _geometry_plans[idx]


def _ctx_for(batch, plan=None) -> Context:
    """Context cached on the batch object (geometry only unless a network plan is given)."""
    plan = plan or geometry_plan(batch["X"].device)
    cache = batch.__dict__.setdefault("_pp_ctx", {}) if hasattr(batch, "__dict__") else {}
    hit = cache.get(id(plan))
    if hit is None or not hit[0].matches(batch):       # tensor identity + version counters (lib.BatchKey), not data_ptr
        cache.clear()
        hit = cache[id(plan)] = (BatchKey(batch), Context(plan, batch))
    return hit[1]


def get_atom14_coords(X, S, BB_D, SC_D):
    lead = X.shape[:-2]
    L = lead[-1]
    b = Batch(X=X.reshape(-1, L, 14, 3), residue_type=S.reshape(-1, L), BB_D=BB_D.reshape(-1, L, 3))
    ctx = Context(geometry_plan(X.device), b)
    return ctx.atom14(SC_D.reshape(-1, L, 4)).reshape(*lead, 14, 3)


def compute_residue_clash(batch, SC_D, violation_tolerance_factor=12., clash_overlap_tolerance=0.5):
    """On a batch with obstacle atoms (``protein_to_batch(..., obstacles=...)``) the clash reported
    includes every side-chain atom's overlap with the obstacles of its complex."""
    return _ctx_for(batch).clash(SC_D, violation_tolerance_factor, clash_overlap_tolerance)


def find_clash_mask(batch, SC_D, violation_tolerance_factor, clash_overlap_tolerance, fixed_mask=None):
    """``fixed_mask`` ([B, L], nonzero = kept): the rows the pinned optimiser moves, the clash mask -- its mean over all rows -- less
    the kept rows.  The clash behind the mask includes obstacle atoms, if the batch carries any."""
    pr = compute_residue_clash(batch, SC_D, violation_tolerance_factor, clash_overlap_tolerance)
    mask = pr > pr.mean()
    if fixed_mask is not None:
        mask = mask & ~(torch.as_tensor(fixed_mask).to(pr.device) != 0).reshape(pr.shape)
    return mask.unsqueeze(-1).expand(-1, -1, 4)


def proximal_optimizer(batch, SC_D, violation_tolerance_factor, clash_overlap_tolerance, lamda,
                       num_steps=50, fixed_mask=None) -> Tuple[List[torch.Tensor], List[float]]:
    """``fixed_mask`` ([1, L], nonzero = kept): the pinned optimiser (pp_proximal_pinned); kept rows are ``SC_D`` bit for bit in
    every entry of the list.  On a batch with obstacle atoms the clash in the mask, the loss and the gradient includes them."""
    assert batch.num_proteins == 1
    ctx = _ctx_for(batch)
    if fixed_mask is None:
        traj, _, losses = ctx.proximal(SC_D, violation_tolerance_factor, clash_overlap_tolerance, lamda, num_steps, want_traj=True)
    else:
        traj, _, _, losses = ctx.proximal_packed(SC_D, violation_tolerance_factor, clash_overlap_tolerance, lamda, num_steps,
                                                 want_traj=True, fixed=fixed_mask)
        losses = losses[0]
    loss_list = [float(v) for v in losses.cpu()]          # the one host sync of the whole optimisation
    return [traj[i] for i in range(num_steps)], loss_list


def solvent_accessibility(batch, SC_D=None, n_points=96, probe=1.4, radius=None, want_counts=False):
    """Solvent-accessible surface of every residue at four nested levels (``lib.Context.sasa``, pp_sasa), on
    the geometry plan: at the angles ``SC_D`` (through atom14), else at the batch's X.  Padded, packed and decoy batches alike: the
    occluders of a row are the rows and the obstacle atoms of its own complex.  Returns ``area`` [B, L, 4], ``seg_area`` fp64
    [n_complexes, 4], ``counts`` (with ``want_counts``), ``bsa``, ``interface``, ``pocket`` and ``exposure``."""
    return _ctx_for(batch).sasa(chi=SC_D, n_points=n_points, probe=probe, radius=radius, want_counts=want_counts)


def polar_contacts(batch, chi=None, hb_max=3.5, sb_max=4.0, want_partners=True, sasa=False, bury_points=0, n_points=96, probe=1.4,
                   obst_polar=None):
    """Hydrogen bonds, salt bridges and unsatisfied polar atoms of every complex (``lib.Context.polar``, pp_polar; DESIGN.md section
    27), on the geometry plan: at the angles ``chi`` (through atom14), else at the batch's X.  Padded, packed and decoy batches alike.
    ``sasa=True`` also runs ``Context.sasa`` at the same coordinates (``n_points``, ``probe``) and fills ``buns`` and
    ``buns_interface``.  ``obst_polar`` [M]: which obstacle atoms are polar, in place of the batch's ``obstacle_polar``."""
    ctx = _ctx_for(batch)
    xyz = ctx.atom14(chi) if chi is not None else None
    sa = ctx.sasa(xyz=xyz, n_points=n_points, probe=probe, want_counts=True) if sasa else None
    return ctx.polar(xyz=xyz, hb_max=hb_max, sb_max=sb_max, want_partners=want_partners, sasa=sa, bury_points=bury_points,
                     obst_polar=obst_polar)


def add_hydrogens(batch, SC_D=None, link=None):
    """The hydrogens of every row, placed on the device (``lib.Context.hydrogens``, pp_hydrogens), on the geometry
    plan: at the angles ``SC_D`` (through atom14), else at the batch's X.  ``link``: the ``partner`` array of ``Context.disulfides``
    (a bonded cysteine has no HG).  Returns ``hxyz`` [B, L, 13, 3], ``hmask`` [B, L, 13], ``link_prev`` [B, L] and ``xyz``."""
    return _ctx_for(batch).hydrogens(chi=SC_D, link=link)


def clashscore(batch, SC_D=None, link=None, rotatable="skip", cut=0.4, hb_allow=0.6, radius=None, want_partners=True):
    """All-atom clashscore of every complex with placed hydrogens (``lib.Context.clashscore``, pp_clashscore), on
    the geometry plan: at the angles ``SC_D`` (through atom14), else at the batch's X.  Padded, packed and decoy batches alike.  Not
    MolProbity's number: this package's radius table; flips and rotatable hydrogens are optimised by ``optimize_hydrogens``, not here."""
    return _ctx_for(batch).clashscore(chi=SC_D, link=link, rotatable=rotatable, cut=cut, hb_allow=hb_allow, radius=radius,
                                      want_partners=want_partners)


def optimize_hydrogens(batch, SC_D=None, link=None, max_sweeps=32, hb_weak=2.5, hb_good=2.2, cut=0.4, hb_allow=0.6, radius=None,
                       obst_polar=None, want_candidates=False):
    """Asn / Gln / His flips and rotatable hydrogens chosen on the device (``lib.Context.hbond_optimize``, pp_hnet_optimize; DESIGN.md
    section 30), on the geometry plan: at the angles ``SC_D`` (flips and rotors), else at the batch's X (rotors alone).  Padded,
    packed and decoy batches alike.  The result goes to ``Context.clashscore(chi=res.chi, hydrogens=res, rotatable="keep")`` as it
    is.  Integer counts of overlaps and explicit-hydrogen bonds, not Reduce's dot scores."""
    return _ctx_for(batch).hbond_optimize(chi=SC_D, link=link, max_sweeps=max_sweeps, hb_weak=hb_weak, hb_good=hb_good, cut=cut,
                                          hb_allow=hb_allow, radius=radius, obst_polar=obst_polar, want_candidates=want_candidates)


def refine_allatom(batch, SC_D, fixed=None, link=None, deltas_deg=(16, 8, 4), max_steps=3, max_sweeps=32, bands=4, band=0.15, cut=0.4,
                   hb_allow=0.6, hb_weak=2.5, hb_good=2.2, radius=None, obst_polar=None, want_candidates=False):
    """Side chains refined in chi space against the explicit-hydrogen overlaps ``clashscore`` counts, on the device
    (``lib.Context.refine_allatom``, pp_chi_refine), on the geometry plan.  Padded, packed and decoy batches
    alike.  A residue without a serious overlap keeps its angles bit for bit; the defaults are starting values, not tuned against
    anything.  ``res.chi`` goes to ``clashscore`` / ``optimize_hydrogens`` as it is."""
    return _ctx_for(batch).refine_allatom(SC_D, fixed=fixed, link=link, deltas_deg=deltas_deg, max_steps=max_steps, max_sweeps=max_sweeps,
                                          bands=bands, band=band, cut=cut, hb_allow=hb_allow, hb_weak=hb_weak, hb_good=hb_good,
                                          radius=radius, obst_polar=obst_polar, want_candidates=want_candidates)


def close_anchors(batch, SC_D, anchor_set, fixed=None, max_energy=10.0, sigma_chi=0.3490658503988659, names=None):
    """Metal sites and covalent links closed on the device (``lib.Context.anchors``, pp_anchor_close), on the
    geometry plan: every anchor of ``anchor_set`` (``selection.AnchorSet``, rows of the batch) -- a distance restraint, optionally
    with an angle term, between a side-chain atom and a fixed point -- is closed next to the angles ``SC_D`` by a grid search over
    the chi angles its donor depends on.  Padded, packed and decoy batches alike.  ``res.chi`` equals ``SC_D`` bit for bit outside
    the closed rows; ``res.pinned()`` is the mask of rows a later stage must keep.  ``sigma_chi`` is 20 degrees in radians."""
    return _ctx_for(batch).anchors(SC_D, anchor_set, fixed=fixed, max_energy=max_energy, sigma_chi=sigma_chi, names=names)


def polar_bond_keys(partners, seg_offsets=None):
    """The hydrogen bonds behind a ``partners`` array of ``Context.polar`` ([B, L, 14, 4], packed [1, N, 14, 4]) as sorted unique int64
    keys ``(segment * M + low code) * M + high code`` with ``M = 14 * rows`` of the array's second axis, on the device.  A bond is in
    the set when either of its atoms lists the other, so an atom with more partners than the list holds loses a bond only if the
    partner's list is full as well.  ``seg_offsets``: the segment table of a packed batch (a list); None: every [L] row of the array
    is a segment.  Returns (keys, M, number of segments).  The values stay on the device, but the number of keys depends on the data
    (a boolean selection and ``torch.unique``): the call waits for the stream."""
    p = partners.reshape(-1, 14, partners.shape[-1]).long()
    n, L = p.shape[0], int(partners.shape[-3])
    dev = p.device
    row = torch.arange(n, device=dev)
    if seg_offsets is None:
        n_seg = n // L
        seg, first = row // L, (row // L) * L
    else:
        offs = torch.as_tensor([int(x) for x in seg_offsets], device=dev)
        n_seg = offs.numel() - 1
        seg = torch.bucketize(row, offs[1:], right=True).clamp(max=n_seg - 1)
        first = offs[seg]
    M = 14 * L
    own = ((row - first) * 14)[:, None, None] + torch.arange(14, device=dev)[None, :, None]
    own = own.expand_as(p)
    lo, hi = torch.minimum(own, p), torch.maximum(own, p)
    key = (seg[:, None, None] * M + lo) * M + hi
    return torch.unique(key[p >= 0]), M, n_seg


def polar_recovery(native, sampled, seg_offsets=None):
    """How many of the native hydrogen bonds with at least one side-chain atom (slot >= 4) a sample has: ``native`` and ``sampled``
    are two ``partners`` arrays of ``Context.polar`` over the same rows (or the results themselves), ``seg_offsets`` the segment
    table of a packed batch.  Returns (native int64 [n_segments], recovered int64 [n_segments]) on the device, computed with
    torch from the bonds either atom lists (``polar_bond_keys``): atoms at the cap of their list are included.  Nothing is copied
    to the host, but the call waits for the stream (the bond sets have data-dependent sizes)."""
    a = native["partners"] if isinstance(native, dict) else native
    b = sampled["partners"] if isinstance(sampled, dict) else sampled
    if a is None or b is None or tuple(a.shape) != tuple(b.shape):
        raise ValueError("polar_recovery: needs two partners arrays of the same shape")
    ka, M, n_seg = polar_bond_keys(a, seg_offsets)
    kb, _, _ = polar_bond_keys(b, seg_offsets)
    side = ((ka % M) % 14 >= 4) | (((ka // M) % M) % 14 >= 4)
    ka = ka[side]
    kept = torch.isin(ka, kb)
    s = ka // (M * M)
    return torch.bincount(s, minlength=n_seg), torch.bincount(s[kept], minlength=n_seg)


def proximal_optimizer_packed(packed_batch, SC_D, violation_tolerance_factor, clash_overlap_tolerance, lamda, num_steps=50,
                              norm_rows=None, want_traj=False, fixed_mask=None, return_moved=False):
    """``proximal_optimizer`` for every complex of a packed batch (``batch.pack``; a B = 1 batch counts as one complex) in the same
    launches, each complex with the reference's per-complex semantics (optimize.py:5-73: its own clash mask, 1/n, loss list) and
    the accept rule of TDiffusionModule.sampling (TorsionalDiffusion.py:296-298) decided on the device.  ``norm_rows``: the row
    count each complex's means divide by (None: its packed length; its padded ``max_size`` reproduces the run on the padded
    batch, whose padding rows pack() dropped).  Returns (trajectory [num_steps, 1, N, 4] or None, last [1, N, 4],
    accepted [1, N, 4], losses [n_complexes, num_steps]), all left on the device.

    ``fixed_mask`` ([1, N], nonzero = kept; pp_proximal_pinned): kept rows leave the clash mask, whose mean stays over all rows of
    the complex, and come out as ``SC_D`` bit for bit; all zero gives the bits of the call without it.  ``return_moved`` appends
    the mask that was optimised (bool [1, N]).  On a batch with obstacle atoms (``batch.pack`` carries them per complex) the clash
    in every mask, loss and gradient includes the obstacles of the row's own complex."""
    return _ctx_for(packed_batch).proximal_packed(SC_D, violation_tolerance_factor, clash_overlap_tolerance, lamda, num_steps,
                                                  norm_rows=norm_rows, want_traj=want_traj, fixed=fixed_mask,
                                                  return_moved=return_moved)
