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
