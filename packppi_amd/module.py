"""``TDiffusionModule``: the reference Lightning module's inference surface on the HIP path.

Mirrors ``src/models/TorsionalDiffusion.py``: ``network`` (:90-109), ``add_sc_noise`` (:111-124),
``sampling`` (:254-298), ``compute_rmsd`` (:300-309), ``analyze_samples`` (:311-341), the plain
``schedule`` attribute (:77) and ``load_from_checkpoint(..., strict=False)`` as the CLIs use it
(eval_diffusion.py:29-41); and the denoising score-matching loss ``forward`` / ``step`` / ``validation_step`` /
``test_step`` (:126-229), forward pass only.  Gradients, optimisers and the other Lightning hooks are out of scope.
"""
import math
import pickle
import zipfile
from types import SimpleNamespace
from typing import Any, Dict, Optional

import numpy as np
import torch

from .functional import proximal_optimizer, proximal_optimizer_packed
from .lib import BatchKey, Context, Plan, _get

SAMPLE_DEFAULTS = dict(eval_epochs=1, sample_during_training=True, annealed_temp=3, mode="ode", use_proximal=True,
                       violation_tolerance_factor=12., clash_overlap_tolerance=0.5, lamda=1., num_steps=50)

SIGMA_MIN, SIGMA_MAX = 0.01 * math.pi, math.pi


def _cfg(obj, defaults):
    out = dict(defaults)
    if obj is not None:
        src = obj if isinstance(obj, dict) else vars(obj)
        out.update({k: v for k, v in src.items() if k in defaults})
    return SimpleNamespace(**out)


class _Stub(dict):
    """Inert stand-in for any class the unpickler cannot import (OmegaConf nodes, Lightning callbacks, ...)."""

    def __init__(self, *a, **k):
        dict.__init__(self)

    def __setstate__(self, state):
        pass

    def __call__(self, *a, **k):
        return _Stub()

    def append(self, x):
        pass

    def extend(self, xs):
        pass

    def add(self, x):
        pass


class _TolerantUnpickler(pickle.Unpickler):
    """Reads a Lightning ``.ckpt`` without Lightning / OmegaConf: unknown classes become inert stubs."""

    def find_class(self, module, name):
        if module.split(".")[0] in ("torch", "collections", "numpy", "builtins", "_codecs"):
            return super().find_class(module, name)
        return _Stub


class _TolerantPickle:
    Unpickler = _TolerantUnpickler
    __name__ = "pickle"

    @staticmethod
    def load(f, **kw):
        return _TolerantUnpickler(f, **kw).load()


def read_checkpoint_state_dict(path, map_location="cpu") -> Dict[str, torch.Tensor]:
    try:
        ckpt = torch.load(path, map_location=map_location, weights_only=True)
    except Exception:
        ckpt = torch.load(path, map_location=map_location, weights_only=False, pickle_module=_TolerantPickle)
    sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
    return {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}


def _corrector_refusals(corrector, schedule, sde_noise, seed):
    """The refusals of ``sampling(corrector=)``, behind every other one: the snr array of ``Context.sample_corrected``."""
    if sde_noise is not None:
        raise ValueError("corrector and sde_noise exclude each other: corrected sampling draws its noise from the seeded generator")
    if seed is None:
        raise ValueError("corrector needs seed: the corrector draws its noise from the seeded generator")
    from .schedule import resolve_corrector
    return resolve_corrector(corrector, schedule)          # snr must be finite and not negative


def _sampling_refusals(cfg, schedule, batch, use_proximal, return_list, sde_noise, seed, fixed_mask, fixed_mode, return_trajectory,
                       guide, corrector=None):
    """Every refusal of ``sampling``, in the order a call with several faults has always met them.  Returns (the guide's keywords
    for ``Context.sample_guided``, None without a guide; the corrector's snr array, None without a corrector)."""
    gkw = None
    if guide is not None:
        from .schedule import resolve_guide
        eta, cap = resolve_guide(guide, schedule)
        if sde_noise is not None:
            raise ValueError("guide and sde_noise exclude each other: guided sde sampling draws its noise from the seeded generator")
        if seed is None and cfg.mode == "sde":
            raise ValueError("guide needs seed in sde mode: the guided sampler draws its noise inside the reverse step")
        if seed is None and fixed_mask is not None:
            raise ValueError("guide with fixed_mask needs seed: the fixed rows are re-noised with the seeded generator's draws")
        if return_trajectory and use_proximal:
            raise ValueError("return_trajectory with guide returns the sampler's trajectory: run the proximal stage separately")
        if _get(batch, "seg_offsets") is None and int(batch.num_proteins) != 1:
            raise ValueError("guide needs a B = 1 batch or a packed one (batch.pack), not a padded B > 1 batch")
        gkw = dict(eta=eta, cap=cap, vtf=cfg.violation_tolerance_factor, tol=cfg.clash_overlap_tolerance)
    if fixed_mask is not None:
        if seed is None:
            raise ValueError("fixed_mask needs seed: the fixed rows are re-noised with the seeded generator's draws")
        if sde_noise is not None:
            raise ValueError("fixed_mask and sde_noise exclude each other: partial repacking draws its own noise")
        if use_proximal:
            raise ValueError("fixed_mask with use_proximal=True is not supported here: this proximal stage has no pin and would "
                             "move the fixed rows; repack(batch, fixed_mask, seed=..., use_proximal=True) runs the pinned one")
        from .lib import FIX_MODES
        if fixed_mode not in FIX_MODES:
            raise ValueError(f"fixed_mode must be one of {sorted(FIX_MODES)}")
        return gkw, None if corrector is None else _corrector_refusals(corrector, schedule, sde_noise, seed)
    if return_trajectory and guide is None and corrector is None:
        raise ValueError("return_trajectory needs fixed_mask (the trajectory is written by the partial sampler)")
    if _get(batch, "seg_offsets") is not None and use_proximal and return_list:
        raise ValueError("return_list=True needs a B = 1 batch; for a packed batch use "
                         "functional.proximal_optimizer_packed (per-complex losses [n_complexes, num_steps])")
    if seed is not None and sde_noise is not None:
        raise ValueError("seed and sde_noise exclude each other: the seeded sampler draws its own noise")
    return gkw, None if corrector is None else _corrector_refusals(corrector, schedule, sde_noise, seed)


def _disulfide_refusals(batch, disulfides, return_trajectory, return_list):
    """The refusals of ``sampling(disulfides=)``, behind every other one.  Returns the row pairs of an explicit request, None for
    "auto" (``Context.disulfides`` checks the rows themselves where the batch is)."""
    if _get(batch, "seg_offsets") is None and int(batch.num_proteins) != 1:
        raise ValueError("disulfides needs a B = 1 batch or a packed one (batch.pack), not a padded B > 1 batch")
    if return_trajectory:
        raise ValueError("return_trajectory with disulfides returns the sampler's trajectory: close the bridges separately "
                         "(Context.disulfides)")
    if return_list:
        raise ValueError("return_list with disulfides is not supported: the pinned proximal stage returns the accepted angles")
    if isinstance(disulfides, str) and disulfides.strip() == "auto":
        return None
    if not isinstance(disulfides, str):
        try:
            pairs = list(disulfides)
        except TypeError:
            raise ValueError('disulfides must be None, "auto", a selection string or a list of residue pairs') from None
        if all(isinstance(a, (int, np.integer)) and isinstance(b, (int, np.integer)) for a, b in pairs):
            return [(int(a), int(b)) for a, b in pairs]                   # rows of the batch
    names = _get(batch, "residue_names")
    if names is None:
        raise ValueError("disulfides by chain and residue number needs batch.residue_names (selection.residue_names(protein)); "
                         "row pairs need nothing")
    from .selection import parse_disulfides
    return parse_disulfides(disulfides, dict(chain_id=[n[0] for n in names], residue_index=[n[1] for n in names]))


def _anchor_refusals(batch, anchors, return_trajectory, return_list):
    """The refusals of ``sampling(anchors=)``, behind every other one, as ``_disulfide_refusals``.  Returns (the ``AnchorSet`` of
    every complex with rows of the batch and the segment it claims, or None entries; whether the request was "auto")."""
    from .selection import AnchorSet, parse_anchors
    seg = _get(batch, "seg_offsets")
    if seg is None and int(batch.num_proteins) != 1:
        raise ValueError("anchors needs a B = 1 batch or a packed one (batch.pack), not a padded B > 1 batch")
    if return_trajectory:
        raise ValueError("return_trajectory with anchors returns the sampler's trajectory: close the anchors separately "
                         "(Context.anchors)")
    if return_list:
        raise ValueError("return_list with anchors is not supported: the pinned proximal stage returns the accepted angles")
    host = _get(batch, "seg_offsets_host")
    offs = [int(x) for x in (host if host is not None else (seg.tolist() if seg is not None else [0, int(batch.max_size)]))]
    n_seg = len(offs) - 1
    auto = isinstance(anchors, str) and anchors.strip() == "auto"
    if isinstance(anchors, AnchorSet):
        sets = [anchors]
    elif isinstance(anchors, (list, tuple)):
        sets = list(anchors)
        if not all(s is None or isinstance(s, AnchorSet) for s in sets):
            raise ValueError('anchors must be None, an AnchorSet, a list of them (None entries allowed), "auto" or a spec string')
    elif isinstance(anchors, str):
        paths = _get(batch, "pdb_path")
        if paths is None:
            raise ValueError(f"anchors={anchors.strip()!r} needs batch.pdb_path: the targets are atoms of the PDB file "
                             "(an AnchorSet needs nothing)")
        names = _get(batch, "residue_names")
        if names is None:
            raise ValueError("anchors from a PDB file needs batch.residue_names (selection.residue_names(protein)): LINK records and "
                             "spec strings name residues by chain and number")
        paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
        if len(paths) != n_seg:
            raise ValueError(f"batch.pdb_path names {len(paths)} files, the batch holds {n_seg} complexes")
        if not auto and n_seg != 1:
            raise ValueError("an anchors spec string names the residues of ONE complex: give a packed batch a list of AnchorSets")
        from .pdb_io import anchor_sites, hetero_atoms
        rt = batch["residue_type"].reshape(-1).cpu().numpy()
        sets = []
        for i, path in enumerate(paths):
            lo, hi = offs[i], offs[i + 1]
            prot = dict(chain_id=np.asarray([n[0] for n in names[lo:hi]]), residue_index=np.asarray([n[1] for n in names[lo:hi]]),
                        aaindex=rt[lo:hi])
            sets.append(anchor_sites(path, prot, "link") if auto else parse_anchors(anchors, prot, hetero_atoms(path)))
    else:
        raise ValueError('anchors must be None, an AnchorSet, a list of them (None entries allowed), "auto" or a spec string')
    if len(sets) != n_seg:
        raise ValueError(f"anchors holds {len(sets)} sets, the batch holds {n_seg} complexes (one set per complex, None for none)")
    return [None if s is None else s.shifted(offs[i], i) for i, s in enumerate(sets)], auto


class TDiffusionModule:
    NUM_CHI_ANGLES = 4
    eps = 1e-6

    def __init__(self, state_dict: Dict[str, torch.Tensor], sample_cfg: Any = None, encoder_cfg: Any = None,
                 model_cfg: Any = None, device="cuda", knn_ties: Optional[str] = None, **kwargs):
        """``encoder_cfg`` / ``model_cfg`` / ``sample_cfg``: what eval_diffusion.py:33-40 instantiates from the YAML files (dicts
        or namespaces; ``config.load_hot_path_configs`` reads them).  The kernels are compiled for the reference's dimensions:
        any other ``hidden_dim`` / ``top_k`` / ``n_points`` / ``num_rbf`` ... raises a RuntimeError naming the key."""
        from .config import check_compiled_dims
        check_compiled_dims(encoder_cfg, model_cfg)
        self._state_dict = {k: v.detach().float().cpu() for k, v in state_dict.items()}
        self.hparams = SimpleNamespace(sample_cfg=_cfg(sample_cfg, SAMPLE_DEFAULTS), encoder_cfg=encoder_cfg,
                                       model_cfg=model_cfg)
        if self.hparams.sample_cfg.mode not in ("ode", "sde"):
            raise NotImplementedError(self.hparams.sample_cfg.mode)
        # schedule.py:216-217 tests `if self.annealed_temp`: 0 and None (Sampling.yaml `annealed_temp: null`) mean weight 1
        if not self.hparams.sample_cfg.annealed_temp:
            self.hparams.sample_cfg.annealed_temp = 0.0
        if not np.isfinite(float(self.hparams.sample_cfg.annealed_temp)):
            raise RuntimeError(f"sample_cfg.annealed_temp = {self.hparams.sample_cfg.annealed_temp!r}: must be a finite number, 0 or null")
        self.schedule = torch.linspace(1, 0, 31)              # schedule.py:286-288
        self.device = torch.device("cpu")
        self._plan: Optional[Plan] = None
        self._ctx_key, self._ctx = None, None
        self._score_norm = None           # [2, 5001] fp64 on the device: set_score_norm, or made at the first forward
        self._knn_ties = knn_ties         # None: the library default (the reference CPU path's torch.topk choice)
        self.keep_guide_trace = False     # True: guided sampling runs append (eta, clash trace) to guide_traces
        self.guide_traces = []
        self.keep_corrector_trace = False     # True: corrected runs append (snr, (s2, n2, eps, amp) on the device) to corrector_traces (section 23)
        self.corrector_traces = []
        self.keep_disulfide_report = False    # True: runs with disulfides= append what Context.disulfides returned (plus chi_before) to disulfide_reports (section 26)
        self.disulfide_reports = []
        self.keep_anchor_report = False       # True: runs with anchors= append what Context.anchors returned (plus the set and chi_before) to anchor_reports (section 34)
        self.anchor_reports = []
        self.to(device)

    # ---- construction ----------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, map_location=None, strict=False, **kwargs):
        sd = read_checkpoint_state_dict(checkpoint_path)
        return cls(sd, device=map_location or "cuda", **kwargs)

    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("packppi_amd.TDiffusionModule runs on the MI355X HIP device only; use the reference "
                               f"implementation for device '{device}'")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self._plan is None or self._plan.device != device:
            self._plan = Plan(self._state_dict, device)
            if self._knn_ties is not None:
                self._plan.set_knn_ties(self._knn_ties)
            self._plan.set_annealed_temp(self.hparams.sample_cfg.annealed_temp)      # Sampling.yaml:4 -> SO2VESchedule
            self._ctx_key, self._ctx = None, None
        self.device = device
        return self

    def eval(self):
        return self

    def state_dict(self):
        return dict(self._state_dict)

    # ---- internals -------------------------------------------------------------------------
    def _key_matches(self, batch) -> bool:
        return self._ctx_key is not None and self._ctx_key.matches(batch)

    def _context(self, batch) -> Context:
        if not self._key_matches(batch):
            self._ctx_key, self._ctx = None, None          # drop the old workspace first: the new context takes it over
            self._ctx = Context(self._plan, batch)
            self._ctx_key = BatchKey(batch)
        return self._ctx

    def _geometry_context(self, batch) -> Context:
        """The batch's network context if it is the cached one, else a weight-free one (atom14 needs no graph or edge
        embedding: metrics of many small complexes must not pay a network preparation each)."""
        if self._key_matches(batch):
            return self._ctx
        from .functional import _ctx_for
        return _ctx_for(batch)

    @staticmethod
    def _t_to_sigma(t):
        lo, hi = np.log(SIGMA_MIN), np.log(SIGMA_MAX)
        return torch.exp(lo + (hi - lo) * t)

    # ---- reference surface -------------------------------------------------------------------
    def network(self, batch, SC_D_noised, t):
        """-> (pred_score [B,L,4], h_V [B,L,128]).  ``t``: one value, or [B*L] (packed batch: [N]); mixed values run the per-row
        embedding kernel (pp_score_rows), one shared value pp_score.  ``t`` is NOT modified: the reference multiplies it by
        10000 in place (layers.py:258), a side effect its own ``forward`` never observes."""
        t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
        return self._context(batch).score(SC_D_noised, t if t.numel() > 1 else float(t[0]))

    @torch.no_grad()
    def add_sc_noise(self, batch, t):
        """Wrapped chi + sigma(t) N(0,1) on the 1pi then 2pi masks; two draws from the global generator of
        the batch's device, in the reference's order.  The second return (the lookup-table score the reference
        computes and sampling discards) is not reproduced: zeros."""
        x = batch.SC_D.reshape(-1, 4)
        sig = self._t_to_sigma(t.to(x.device)).unsqueeze(-1)
        n1 = torch.randn_like(x) * sig
        x = x + n1 * batch.chi_1pi_periodic_mask.reshape(-1, 4)
        n2 = torch.randn_like(x) * sig
        x = x + n2 * batch.chi_2pi_periodic_mask.reshape(-1, 4)
        x = (x + np.pi) % (2 * np.pi) - np.pi
        shape = (batch.num_proteins, -1, 4)
        return x.reshape(shape), torch.zeros_like(x).reshape(shape)

    @torch.no_grad()
    def add_sc_noise_with_score(self, batch, t, noise=None):
        """``add_sc_noise`` with its second return: (noised angles, target score), TorsionalDiffusion.py:111-124.  The same two
        draws in the same order (or ``noise`` [2, N, 4], the two N(0,1) draws, injected); the target score of each schedule is
        SO2Schedule.score(noise, sigma) (schedule.py:185-193) computed on the device without the tables, masked like the
        noise, and joined as ``where(1pi mask, score_1pi, score_2pi)``."""
        from .lib import so2_score
        x = batch.SC_D.reshape(-1, 4)
        sig = self._t_to_sigma(t.to(x.device)).unsqueeze(-1)
        m1, m2 = batch.chi_1pi_periodic_mask.reshape(-1, 4), batch.chi_2pi_periodic_mask.reshape(-1, 4)
        if noise is not None:
            noise = torch.as_tensor(noise).to(device=x.device, dtype=x.dtype)
            if tuple(noise.shape) != (2, *x.shape):
                raise ValueError(f"noise must have shape {(2, *x.shape)} (the 1pi draw, then the 2pi draw), got {tuple(noise.shape)}")
        n1 = (torch.randn_like(x) if noise is None else noise[0]) * sig
        s1 = so2_score(n1, sig, True) * m1
        x = x + n1 * m1
        n2 = (torch.randn_like(x) if noise is None else noise[1]) * sig
        s2 = so2_score(n2, sig, False) * m2
        x = x + n2 * m2
        x = (x + np.pi) % (2 * np.pi) - np.pi
        shape = (batch.num_proteins, -1, 4)
        return x.reshape(shape), torch.where(m1.bool(), s1, s2).reshape(shape)

    # ---- denoising score-matching loss (TorsionalDiffusion.py:126-229) -----------------------------------------------------------
    def set_score_norm(self, tables=None, seed=None):
        """The two ``score_norm_`` tables the loss divides by.  ``tables``: an ``.npy`` path or a [2, 5001] array (1pi, 2pi), e.g.
        from a reference run; None: ``schedule.score_norm_tables(seed)`` (seed None: unseeded np.random, as the reference)."""
        from .schedule import load_score_norm, score_norm_tables
        arr = load_score_norm(tables) if tables is not None else score_norm_tables(seed, self.device)
        self._score_norm = torch.from_numpy(np.ascontiguousarray(arr)).to(self.device)
        return self

    def _segments(self, batch):
        offs = _get(batch, "seg_offsets_host")
        if offs is None and _get(batch, "seg_offsets") is not None:
            offs = [int(v) for v in _get(batch, "seg_offsets").tolist()]
        if offs is not None:
            return [b - a for a, b in zip(offs[:-1], offs[1:])]
        return [int(batch.max_size)] * int(batch.num_proteins)

    @torch.no_grad()
    def forward(self, batch, t=None, noise=None, per_complex=False):
        """The loss ``trainer.test`` / every validation epoch report: fp64 scalar ``sum num / max(sum den, 1)`` over the batch
        (TorsionalDiffusion.py:126-154); ``per_complex=True``: [n_complexes] ``num / max(den, 1)``.  ``t``: one time per complex
        ([num_proteins]; packed batch: one per packed complex), None draws ``torch.rand`` on the CPU like ``sample_train_t``.
        ``noise``: the two N(0,1) draws [2, N, 4], None draws them on the batch's device."""
        lens = self._segments(batch)
        if t is None:
            t = torch.rand((len(lens),))
        t = torch.as_tensor(t, dtype=torch.float32).reshape(-1)
        if t.numel() != len(lens):
            raise ValueError(f"t has {t.numel()} entries for {len(lens)} complexes (one time per complex)")
        if self._score_norm is None:
            self.set_score_norm()
        self._score_norm = self._score_norm.to(self.device)
        t_rows = torch.repeat_interleave(t, torch.tensor(lens)).to(self.device)
        SC_D_noised, target = self.add_sc_noise_with_score(batch, t_rows, noise)
        ctx = self._context(batch)
        pred, _ = ctx.score_rows(SC_D_noised, t_rows)
        num, den = ctx.dsm_loss(pred, target, t_rows, self._score_norm)
        if per_complex:
            return num / den.clamp(min=1)
        return num.sum() / den.sum().clamp(min=1)

    def step(self, batch):
        return self.forward(batch)

    def _metric_step(self, name, batch):
        loss = self.step(batch)
        tot, n = getattr(self, "_" + name, (0.0, 0))
        setattr(self, "_" + name, (tot + float(loss), n + 1))
        return {"loss": loss}

    def validation_step(self, batch, batch_idx=0):
        return self._metric_step("val_loss", batch)

    def test_step(self, batch, batch_idx=0):
        return self._metric_step("test_loss", batch)

    @property
    def val_loss(self) -> float:
        """Running mean of the ``validation_step`` losses (``reset_metrics`` clears it); NaN before the first step."""
        tot, n = getattr(self, "_val_loss", (0.0, 0))
        return tot / n if n else float("nan")

    @property
    def test_loss(self) -> float:
        tot, n = getattr(self, "_test_loss", (0.0, 0))
        return tot / n if n else float("nan")

    def reset_metrics(self):
        self._val_loss, self._test_loss = (0.0, 0), (0.0, 0)

    def sampling(self, batch, use_proximal: bool = False, return_list: bool = False, sde_noise=None, seed=None,
                 fixed_mask=None, fixed_chi=None, fixed_mode="renoise", return_trajectory: bool = False, guide=None, corrector=None,
                 disulfides=None, refine_allatom: bool = False, anchors=None):
        """``seed`` (an int, None = the reference's behaviour): the initial noising and the sde noise come from the counter-based
        generator on the device (csrc/pp_rng.h) instead of torch's global one.  The noise of a complex is then a function of
        (seed, its key, its rows, the step) alone: the same complex gets the same angles alone, anywhere in a packed batch and
        on any rank.  Keys: ``batch.complex_keys`` (a list or int64 tensor, one per complex; ``batch.pack`` collects them from the
        complexes' ``complex_key``), else 0, 1, 2 ... in batch order.  This is not torch's stream: a seeded run does not
        reproduce a reference run under the same ``torch.manual_seed``.

        ``fixed_mask`` (bool / uint8 [B, L], packed batch: [1, N]; 1 = keep; default ``batch.fixed_mask`` if the batch carries one):
        partial repacking -- those rows keep ``fixed_chi`` (default ``batch.SC_D``), the others are sampled around them
        (DESIGN.md section 13).  ``fixed_mode``: "renoise" (replacement conditioning: at every step the network sees the fixed rows
        noised to that step's level) or "hold" (it sees them clean throughout).  Needs ``seed``; fixed rows of the result are
        ``fixed_chi`` bit for bit.  ``return_trajectory``: (sample, angles after every step [n_steps, B, L, 4]).

        Obstacle atoms (a batch from ``protein_to_batch(..., obstacles=...)``): the network does not see
        them, the sample is what it is without them; with ``use_proximal`` the clash the proximal stage reports and optimises
        includes every side-chain atom's overlap with the obstacles of its complex.

        ``guide`` (None = today's code path, untouched): clash-guided sampling -- a gradient step on the clash
        loss, obstacle atoms included, in front of the network evaluations and behind the last reverse step
        (``Context.sample_guided``).  A number is the step size of the default preset (``schedule.GUIDE_DEFAULTS``: nudges from
        t = 0.3 on, at most 0.1 rad per angle and nudge -- starting values, not tuned ones), a dict holds any of ``scale``, ``kind``
        ("late" / "constant"), ``t_on``, ``cap``, anything else is an explicit sequence of n_schedule step sizes.  Needs ``seed`` in
        sde mode and with ``fixed_mask`` (fixed rows are never nudged); excludes ``sde_noise``; a packed or B = 1 batch.  With
        ``return_trajectory``: (sample, angles after every reverse step, mean clash in front of every nudge, fp64
        [n_complexes, n_schedule], NaN where no nudge runs).  ``use_proximal`` runs behind it, as today.

        ``corrector`` (None = today's code path, untouched): predictor-corrector sampling -- one Langevin
        corrector behind the reverse steps (``Context.sample_corrected``): one more network evaluation at the new state, then a
        step along the score plus noise, with a step size PER COMPLEX from the ratio of its noise norm to its score norm (the
        reference's ``step_correct`` averages the norms over the batch; here batching changes no result).  A number is the snr of
        the default preset (``schedule.CORRECTOR_DEFAULTS``: behind every reverse step but the last; 0.16 is the reference's
        constant, not a tuned one), a dict holds any of ``snr``, ``t_on``, ``last``, anything else is an explicit sequence of
        n_schedule - 1 values.  Needs ``seed``; excludes ``sde_noise``; works with ``fixed_mask`` (fixed rows are never moved and
        never counted) and with ``guide``.  With ``return_trajectory`` the tuple ends with (s2, n2, eps, amp) per complex and step,
        fp64 [n_complexes, n_steps, 4], NaN where no corrector ran; the trajectory holds the angles IN FRONT OF each corrector.

        ``disulfides`` (None = today's code path, untouched): close disulfide bridges behind the sampler (and
        behind guide and corrector) -- ``Context.disulfides`` sets the chi1 of every bonded cysteine pair next to the sample.  "auto":
        detect the pairs from the backbone; a list of row pairs ``(a, b)``; or pairs by name, a list of ``((chain, number), (chain,
        number))`` or a string ``A:5-A:55,...`` (needs ``batch.residue_names``, from ``selection.residue_names(protein)``).  With
        ``use_proximal`` the bridges are closed first and the proximal stage then runs PINNED on the bonded rows
        (``proximal_optimizer_packed(..., fixed_mask=)``), so that its accept rule cannot reopen one.  Rows of ``fixed_mask`` keep
        their chi1.  A packed or B = 1 batch; excludes ``return_trajectory`` and ``return_list``.  ``keep_disulfide_report`` appends
        every run's result to ``disulfide_reports``.

        ``refine_allatom`` (False = today's code path, untouched): behind the proximal stage and the disulfide
        closure, ONE ``Context.refine_allatom`` over the rows of the batch lowers the explicit-hydrogen overlaps in chi space.  Rows
        of ``fixed_mask`` and bonded cysteines stay; a residue without a serious overlap keeps its angles bit for bit.  Excludes
        ``return_trajectory`` and ``return_list``.  ``keep_refine_report`` appends every run's result to ``refine_reports``.

        ``anchors`` (None = today's code path, untouched): close metal sites and covalent links behind the
        sampler and behind the disulfide closure -- ``Context.anchors`` sets the chi angles each anchored donor depends on next to the
        sample.  An ``AnchorSet`` (``selection.AnchorSet``; rows of its complex), a list of them with one per complex of a packed
        batch (None entries allowed), "auto" (the LINK records of ``batch.pdb_path``; needs ``batch.residue_names``) or a spec string
        ``A:94:NE2=A:301:ZN,...`` (one complex; needs both too).  With ``use_proximal`` the proximal stage runs PINNED on the bonded,
        closed and kept rows and those of ``fixed_mask``; ``refine_allatom`` holds the same rows.  Rows of ``fixed_mask`` keep their
        angles (status 2).  An anchor on a row a bridge has bonded is refused when it was given explicitly, skipped with a warning
        under "auto".  A packed or B = 1 batch; excludes ``return_trajectory`` and ``return_list``.  ``keep_anchor_report`` appends
        every run's result to ``anchor_reports``."""
        if fixed_mask is None:
            fixed_mask = _get(batch, "fixed_mask")
        if refine_allatom and (return_trajectory or return_list):
            raise ValueError("refine_allatom returns the refined angles alone: it excludes return_trajectory and return_list")
        gkw, snr = _sampling_refusals(self.hparams.sample_cfg, self.schedule, batch, use_proximal, return_list, sde_noise, seed,
                                      fixed_mask, fixed_mode, return_trajectory, guide, corrector)
        pairs = _disulfide_refusals(batch, disulfides, return_trajectory, return_list) if disulfides is not None else None
        sets = _anchor_refusals(batch, anchors, return_trajectory, return_list) if anchors is not None else None
        ctx = self._context(batch)
        init, sde_noise, pin = self._initial_angles(ctx, batch, sde_noise, seed, fixed_mask, fixed_chi, fixed_mode)
        out = self._run_sampler(ctx, init, sde_noise, seed, pin, return_trajectory, gkw, snr)
        if return_trajectory:
            return out
        if anchors is not None:
            out, link, held = self._anchor_tail(batch, ctx, out, sets, disulfides, pairs, fixed_mask, use_proximal)
            return self._refine_tail(batch, out, held, link)[0] if refine_allatom else out
        link = None
        if disulfides is not None:
            out, link = self._disulfide_tail(batch, ctx, out, pairs, fixed_mask, use_proximal, want_link=True)
        else:
            out = self._proximal_tail(batch, out, use_proximal, return_list)
        return self._refine_tail(batch, out, fixed_mask, link)[0] if refine_allatom else out

    def _refine_tail(self, batch, chi, fixed_mask=None, link=None):
        """Behind everything else that moves a side chain: ONE ``Context.refine_allatom`` over the rows of ``batch`` (DESIGN.md section
        32), the rows of ``fixed_mask`` and the bonded cysteines of ``link`` held.  Returns (the refined angles, the result)."""
        res = self._context(batch).refine_allatom(chi, fixed=fixed_mask, link=link)
        if getattr(self, "keep_refine_report", False):
            self.__dict__.setdefault("refine_reports", []).append(res)
        return res.chi, res

    @staticmethod
    def _refine_columns(ctx, res):
        """What ``return_all`` gains from a refinement: ``refine_moved`` int64 [n_segments] (rows moved) and ``refine_F`` int64
        [n_segments, 2] (the all-atom overlap energy before and after)."""
        seg_of_row = ctx.hnet_tables().seg_of_row
        moved = torch.zeros(ctx.n_segments, dtype=torch.int64, device=seg_of_row.device).index_add_(0, seg_of_row, res.moved.reshape(-1).to(torch.int64))
        return dict(refine_moved=moved, refine_F=res.F)

    def _disulfide_tail(self, batch, ctx, chi, pairs, fixed_mask, use_proximal, norm_rows=None, want_link=False):
        """Behind the sampler of a run with ``disulfides``: close the bridges (``pairs`` None: detect them), then, with
        ``use_proximal``, the pinned proximal stage on the bonded rows plus the caller's fixed rows.  ``want_link``: (angles, the
        partner array of the closure)."""
        names = _get(batch, "residue_names")
        res = ctx.disulfides(chi=chi, fixed=fixed_mask, pairs=pairs, names=None if names is None else [f"{c}:{n}" for c, n in names])
        if self.keep_disulfide_report:
            self.disulfide_reports.append(dict(partner=res.partner, report=res.report, count=res.count, chi_before=chi,
                                               chi_after=res.chi))
        if not use_proximal:
            return (res.chi, res.partner) if want_link else res.chi
        pinned = (res.partner >= 0).reshape(1, -1)
        if fixed_mask is not None:
            pinned = pinned | (torch.as_tensor(fixed_mask).to(pinned.device) != 0).reshape(1, -1)
        cfg = self.hparams.sample_cfg
        out = proximal_optimizer_packed(batch, res.chi, cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance, cfg.lamda,
                                        cfg.num_steps, norm_rows=norm_rows, fixed_mask=pinned)[2]
        return (out, res.partner) if want_link else out

    def _anchor_tail(self, batch, ctx, chi, sets, disulfides, pairs, fixed_mask, use_proximal, norm_rows=None):
        """Behind the sampler of a run with ``anchors``: the disulfide closure if ``disulfides`` asks for one, then the anchor
        closure, then, with ``use_proximal``, the pinned proximal stage with the bonded, closed and kept rows and the caller's fixed
        rows held.  ``sets``: what ``_anchor_refusals`` returned.  Returns (angles, the partner array of the bridges or None, the held
        rows as a bool [1, N] mask on the device)."""
        sets, auto = sets
        names = _get(batch, "residue_names")
        nm = None if names is None else [f"{c}:{n}" for c, n in names]
        link, held = None, None
        if disulfides is not None:
            res = ctx.disulfides(chi=chi, fixed=fixed_mask, pairs=pairs, names=nm)
            if self.keep_disulfide_report:
                self.disulfide_reports.append(dict(partner=res.partner, report=res.report, count=res.count, chi_before=chi,
                                                   chi_after=res.chi))
            chi, link, held = res.chi, res.partner, (res.partner >= 0).reshape(1, -1)
            bonded = set(held.reshape(-1).nonzero().reshape(-1).tolist())
            kept_sets = []
            for s in sets:
                hit = [] if s is None else [i for i, r in enumerate(s.rows.tolist()) if r in bonded]
                if hit and not auto:
                    r = int(s.rows[hit[0]])
                    raise ValueError(f"anchors: anchor {s.labels[hit[0]] or hit[0]}: {nm[r] if nm is not None else f'row {r}'} is bonded "
                                     "in a disulfide bridge; a row takes one or the other")
                if hit:
                    import warnings
                    warnings.warn(f"anchors: {len(hit)} LINK anchor(s) on cysteines a disulfide bridge has bonded are skipped "
                                  f"({', '.join(s.labels[i] for i in hit)})")
                    s = s.subset([i for i in range(len(s)) if i not in hit])
                kept_sets.append(s)
            sets = kept_sets
        ares = ctx.anchors(chi, sets, fixed=fixed_mask, names=nm)
        if self.keep_anchor_report:
            from .selection import AnchorSet
            self.anchor_reports.append(dict(status=ares.status, report=ares.report, anchor_report=ares.anchor_report, count=ares.count,
                                            chi_before=chi, chi_after=ares.chi, anchors=AnchorSet.concat([s for s in sets if s is not None])))
        pinned = ares.pinned().reshape(1, -1)
        if held is not None:
            pinned = pinned | held
        if fixed_mask is not None:
            pinned = pinned | (torch.as_tensor(fixed_mask).to(pinned.device) != 0).reshape(1, -1)
        out = ares.chi
        if use_proximal:
            cfg = self.hparams.sample_cfg
            out = proximal_optimizer_packed(batch, out, cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance, cfg.lamda,
                                            cfg.num_steps, norm_rows=norm_rows, fixed_mask=pinned)[2]
        return out, link, pinned

    def _initial_angles(self, ctx, batch, sde_noise, seed, fixed_mask, fixed_chi, fixed_mode):
        """(the angles noised to t = 1, the sde noise tensor of an unseeded run or None, the pin's keywords or None).  Seeded: the
        device generator's draws under the batch's keys; with a pin the fixed rows start from ``fixed_chi``, noised like the others
        ("renoise") or clean ("hold").  Unseeded: torch's global generator, call for call as the reference draws."""
        if seed is not None:
            ctx.set_rng_keys(_get(batch, "complex_keys"))
        if fixed_mask is not None:
            fx = (torch.as_tensor(fixed_mask).to(self.device) != 0).reshape(ctx.B, ctx.L)
            ref = ctx._chi(batch.SC_D if fixed_chi is None else fixed_chi)
            init = ctx.add_noise(torch.where(fx.unsqueeze(-1), ref, ctx._chi(batch.SC_D)), 1.0, seed)
            if fixed_mode == "hold":
                init = torch.where(fx.unsqueeze(-1), ref, init)
            return init, None, dict(chi_ref=ref, fixed=fx, fix_mode=fixed_mode)
        if seed is not None:
            return ctx.add_noise(batch.SC_D, 1.0, seed), None, None
        t = torch.tensor([1.]).repeat_interleave(batch.max_size * batch.num_proteins).to(self.device)
        init, _ = self.add_sc_noise(batch, t)
        if self.hparams.sample_cfg.mode == "sde" and sde_noise is None:
            # the reference draws torch.normal(size=[B*L, 4], device=...) inside the loop, once per schedule and step, the
            # 1pi schedule first (schedule.py:225, TorsionalDiffusion.py:271-274): the same calls in the same order, so a
            # seed gives the stream it gives the reference on this device (one [n, 2, N, 4] draw would not)
            shape = (batch.num_proteins * batch.max_size, 4)
            sde_noise = torch.stack([torch.stack([torch.normal(mean=0, std=1, size=shape, device=self.device)
                                                  for _ in range(2)]) for _ in range(len(self.schedule) - 1)])
        return init, sde_noise, None

    def _run_sampler(self, ctx, init, sde_noise, seed, pin, return_trajectory, gkw, snr=None):
        """The reverse diffusion on the context: corrected, guided, pinned, seeded or from the caller's noise tensor, each through
        its export."""
        mode = self.hparams.sample_cfg.mode
        if snr is not None:
            return self._corrected(ctx, init, seed, snr, return_trajectory, gkw, **(pin or {}))
        if gkw is not None:
            return self._guided(ctx, init, seed, return_trajectory, **(pin or {}), **gkw)
        if pin is not None:
            return ctx.sample_partial(init, pin["chi_ref"], pin["fixed"], self.schedule, mode, seed, pin["fix_mode"],
                                      trajectory=return_trajectory)
        return ctx.sample(init, self.schedule, mode, sde_noise, seed=seed)

    def _proximal_tail(self, batch, SC_D_sample, use_proximal, return_list):
        if not use_proximal:
            return SC_D_sample
        cfg = self.hparams.sample_cfg
        if _get(batch, "seg_offsets") is not None:            # every complex optimised on its own terms, accept rule per complex on the device
            return proximal_optimizer_packed(batch, SC_D_sample, cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance,
                                             cfg.lamda, cfg.num_steps)[2]
        SC_D_resample_list, loss_list = proximal_optimizer(batch, SC_D_sample, cfg.violation_tolerance_factor,
                                                           cfg.clash_overlap_tolerance, cfg.lamda, cfg.num_steps)
        if return_list:
            return SC_D_sample, SC_D_resample_list, loss_list
        if loss_list[-1] < loss_list[0]:
            return SC_D_resample_list[-1]
        return SC_D_sample

    def _guided(self, ctx, init, seed, return_trajectory, **kw):
        """``Context.sample_guided`` for ``sampling``: the sample, with ``return_trajectory`` (sample, trajectory, clash trace).
        With ``keep_guide_trace`` set every guided run also appends (eta, clash trace on the device) to ``guide_traces`` (the
        command lines write guide.csv from it); otherwise no trace launch is enqueued unless the caller asked for it."""
        keep = self.keep_guide_trace
        out = ctx.sample_guided(init, self.schedule, self.hparams.sample_cfg.mode, seed, trajectory=return_trajectory,
                                want_trace=return_trajectory or keep, **kw)
        if keep:
            self.guide_traces.append((kw["eta"], out[-1]))
        if return_trajectory:
            return out
        return out[0] if keep else out

    def _corrected(self, ctx, init, seed, snr, return_trajectory, gkw, **pin):
        """``Context.sample_corrected`` for ``sampling``: the sample; with ``return_trajectory`` (sample, trajectory, the clash trace
        of a guided run, corrector trace).  ``keep_guide_trace`` / ``keep_corrector_trace`` append to ``guide_traces`` /
        ``corrector_traces`` as ``_guided`` does (the command lines write guide.csv and corrector.csv from them)."""
        keep_g, keep_c = self.keep_guide_trace and gkw is not None, self.keep_corrector_trace
        want_g, want_c = gkw is not None and (return_trajectory or keep_g), return_trajectory or keep_c
        out = ctx.sample_corrected(init, self.schedule, self.hparams.sample_cfg.mode, seed, snr, trajectory=return_trajectory,
                                   want_trace=want_g, want_corr=want_c, **pin, **(gkw or {}))
        if keep_c:
            self.corrector_traces.append((snr, out[-1]))
        if keep_g:
            self.guide_traces.append((gkw["eta"], out[-2 if want_c else -1]))
        if return_trajectory:
            return out
        return out[0] if isinstance(out, tuple) else out

    def repack(self, batch, fixed_mask=None, *, seed, fixed_chi=None, fixed_mode="renoise", use_proximal: bool = False,
               return_list: bool = False, norm_rows=None, guide=None, corrector=None, disulfides=None, refine_allatom: bool = False,
               anchors=None):
        """Partial repacking in one call (DESIGN.md sections 13 and 14): ``sampling(batch, seed=seed, fixed_mask=...)`` -- the rows
        of ``fixed_mask`` (default ``batch.fixed_mask``) keep ``fixed_chi`` (default ``batch.SC_D``), the others are sampled around
        them -- and then, with ``use_proximal``, the PINNED proximal stage (pp_proximal_pinned): the clash mask of every complex, its
        mean over all of the complex's rows, less the kept rows; the accept rule of ``sampling`` per complex, on the device.  A B = 1
        batch or a packed one (``batch.pack``); ``norm_rows`` as in ``functional.proximal_optimizer_packed`` (the sharded driver passes
        the padded sizes).  Kept rows of the result are ``fixed_chi`` bit for bit with or without the proximal stage.  On a batch with
        obstacle atoms the clash of the pinned stage -- mask, loss, gradient -- includes them.
        ``return_list`` (B = 1, with ``use_proximal``): (sample, per-step angles, losses) as ``sampling`` returns them.
        ``guide``: as in ``sampling`` (clash-guided sampling of the free rows); None = today's path.  ``corrector``: as in ``sampling``.
        ``disulfides``: as in ``sampling`` -- a kept row never changes its chi1, a bridge between two kept rows
        is only reported; the pinned stage then also keeps the bonded rows.
        ``refine_allatom``: as in ``sampling``, behind the pinned stage; kept rows stay kept.
        ``anchors``: as in ``sampling`` -- an anchor on a kept row is only reported (status 2); the pinned stage
        then also keeps the closed rows."""
        if fixed_mask is None:
            fixed_mask = _get(batch, "fixed_mask")
        if refine_allatom and return_list:
            raise ValueError("refine_allatom returns the refined angles alone: it excludes return_list")
        if fixed_mask is None:
            raise ValueError("repack needs fixed_mask (or a batch that carries one); sampling() samples every row")
        packed = _get(batch, "seg_offsets") is not None
        if return_list and (packed or not use_proximal):
            raise ValueError("return_list=True needs use_proximal=True and a B = 1 batch; for a packed batch use "
                             "functional.proximal_optimizer_packed (per-complex losses [n_complexes, num_steps])")
        cfg = self.hparams.sample_cfg
        if anchors is not None:
            pairs = _disulfide_refusals(batch, disulfides, False, return_list) if disulfides is not None else None
            sets = _anchor_refusals(batch, anchors, False, return_list)
            SC_D_sample = self.sampling(batch, seed=seed, fixed_mask=fixed_mask, fixed_chi=fixed_chi, fixed_mode=fixed_mode, guide=guide,
                                        corrector=corrector)
            out, link, held = self._anchor_tail(batch, self._context(batch), SC_D_sample, sets, disulfides, pairs, fixed_mask, use_proximal,
                                                norm_rows)
            return self._refine_tail(batch, out, held, link)[0] if refine_allatom else out
        if disulfides is not None:
            pairs = _disulfide_refusals(batch, disulfides, False, return_list)
            SC_D_sample = self.sampling(batch, seed=seed, fixed_mask=fixed_mask, fixed_chi=fixed_chi, fixed_mode=fixed_mode, guide=guide,
                                        corrector=corrector)
            out, link = self._disulfide_tail(batch, self._context(batch), SC_D_sample, pairs, fixed_mask, use_proximal, norm_rows, want_link=True)
            return self._refine_tail(batch, out, fixed_mask, link)[0] if refine_allatom else out
        SC_D_sample = self.sampling(batch, seed=seed, fixed_mask=fixed_mask, fixed_chi=fixed_chi, fixed_mode=fixed_mode, guide=guide, corrector=corrector)
        if not use_proximal:
            return self._refine_tail(batch, SC_D_sample, fixed_mask)[0] if refine_allatom else SC_D_sample
        traj, _, accepted, losses = proximal_optimizer_packed(batch, SC_D_sample, cfg.violation_tolerance_factor,
                                                              cfg.clash_overlap_tolerance, cfg.lamda, cfg.num_steps,
                                                              norm_rows=norm_rows, want_traj=return_list, fixed_mask=fixed_mask)
        if return_list:
            return SC_D_sample, [traj[i] for i in range(cfg.num_steps)], [float(v) for v in losses[0].cpu()]
        return self._refine_tail(batch, accepted, fixed_mask)[0] if refine_allatom else accepted

    def _recombine(self, ctx, chi, n_decoys, res, recombine_sweeps):
        """``Context.ensemble_recombine`` from the decoy ``ensemble_reduce`` selected (``res.best``, taken on the device) with the
        clash parameters of the sampling configuration, and the keys it adds to a ``return_all`` dict."""
        cfg = self.hparams.sample_cfg
        rec = ctx.ensemble_recombine(chi, n_decoys, start=res.best, max_sweeps=recombine_sweeps,
                                     vtf=cfg.violation_tolerance_factor, tol=cfg.clash_overlap_tolerance)
        return rec, dict(recombined=rec.chi, pick=rec.pick, clash_trace=rec.clash_trace, sweeps=rec.sweeps, converged=rec.converged)

    @staticmethod
    def _decoy_bsa(ctx, chi):
        """fp64 [n_segments]: the surface every segment (decoy) buries between its chains at ``chi``."""
        seg = ctx.sasa(chi=chi).seg_area
        return seg[:, 1] - seg[:, 2]

    @staticmethod
    def _check_select(select):
        from .lib import SELECT
        if select not in SELECT:
            raise ValueError(f"select must be one of 'clash', 'medoid' or None, got {select!r}")

    @staticmethod
    def _decoy_polar(ctx, packed, chi, sasa):
        """The polar contacts of every segment (decoy) at ``chi``, ONE pp_polar over the packed decoys: int32
        [n_segments] ``hbonds``, ``hbonds_interface`` and ``salt_interface`` (columns 0, 1 and 5 of ``Context.polar().seg``) and, with
        ``sasa``, ``buns_interface`` int64 [n_segments] (buried unsatisfied polar atoms that the isolated chain exposes) and ``bsa``.
        The polar obstacle atoms are those the packed batch carries (``obstacle_polar``, per group like the obstacles)."""
        xyz = ctx.atom14(chi)
        sa = ctx.sasa(xyz=xyz, want_counts=True) if sasa else None
        pol = ctx.polar(xyz=xyz, want_partners=False, sasa=sa)
        out = dict(hbonds=pol.seg[:, 0], hbonds_interface=pol.seg[:, 1], salt_interface=pol.seg[:, 5])
        if sasa:
            offs = packed.seg_offsets_host
            lens = torch.tensor([b - a for a, b in zip(offs[:-1], offs[1:])], device=xyz.device)
            seg_of_row = torch.repeat_interleave(torch.arange(len(offs) - 1, device=xyz.device), lens, output_size=offs[-1])
            per_row = pol.buns_interface.reshape(-1, 14).sum(1)
            out["buns_interface"] = torch.zeros(len(offs) - 1, dtype=torch.int64, device=xyz.device).index_add_(0, seg_of_row, per_row)
            out["bsa"] = sa.seg_area[:, 1] - sa.seg_area[:, 2]
        return out

    @staticmethod
    def _decoy_clashscore(ctx, chi):
        """The all-atom clashscore of every segment (decoy) at ``chi``, ONE ``Context.clashscore`` over the packed
        decoys: ``clashscore`` fp64 [n_segments] and ``clashes_interface`` int32 [n_segments] (serious overlaps between chains)."""
        res = ctx.clashscore(chi=chi, want_partners=False)
        return dict(clashscore=res.clashscore, clashes_interface=res.seg[:, 2])

    @staticmethod
    def _decoy_hnet(ctx, chi, clashscore):
        """The hydrogen-bond networks of every segment (decoy) at ``chi`` optimised, ONE ``Context.hbond_optimize``
        over the packed decoys: ``hnet_bonds`` and ``hnet_flips`` int64 [n_segments] (explicit-hydrogen bonds of the movers, rows
        flipped) and, with ``clashscore``, ``clashscore_hnet`` fp64 [n_segments]: the score of the optimised structure with the
        rotatable hydrogens counted."""
        res = ctx.hbond_optimize(chi=chi)
        out = dict(hnet_bonds=res.n_bonds, hnet_flips=res.n_flips)
        if clashscore:
            out["clashscore_hnet"] = ctx.clashscore(chi=res.chi, hydrogens=res, rotatable="keep", want_partners=False).clashscore
        return out

    def _reduce_ensemble(self, packed, chi, select, return_all, recombine, recombine_sweeps, sasa, polar=False, clashscore=False,
                         hbond_optimize=False, refine=None):
        """What the two ensemble calls do with the decoys' angles: the per-residue clash, ``Context.ensemble_reduce``, the
        recombination, the buried surface and the polar contacts if asked for; the selected (or recombined) angles, or the
        ``return_all`` dict."""
        cfg = self.hparams.sample_cfg
        ctx, D = self._context(packed), int(packed.n_decoys)
        per_res = ctx.clash(chi, cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance)
        res = ctx.ensemble_reduce(chi, D, per_res=per_res, select=select)
        rec, extra = self._recombine(ctx, chi, D, res, recombine_sweeps) if recombine else (None, {})
        if polar and return_all:
            extra = dict(extra, **self._decoy_polar(ctx, packed, chi, sasa))
        elif sasa and return_all:
            extra = dict(extra, bsa=self._decoy_bsa(ctx, chi))
        if clashscore and return_all:
            extra = dict(extra, **self._decoy_clashscore(ctx, chi))
        if refine is not None and return_all:
            extra = dict(extra, **self._refine_columns(ctx, refine))
        if hbond_optimize and return_all:
            extra = dict(extra, **self._decoy_hnet(ctx, chi, clashscore))
        if not return_all:
            return rec.chi if recombine else res.chi_best
        return dict(decoys=(chi, packed), selected=res.chi_best, best=res.best, dev=res.dev, clash=res.clash, consensus=res.mean,
                    confidence=res.resultant, keys=list(packed.complex_keys), **extra)

    def sample_ensemble(self, batch, n_decoys, *, seed=None, use_proximal: bool = False, select="clash", return_all: bool = False,
                        recombine: bool = False, recombine_sweeps: int = 64, sasa: bool = False, guide=None, corrector=None,
                        polar: bool = False, clashscore: bool = False, hbond_optimize: bool = False, refine_allatom: bool = False):
        """``n_decoys`` seeded samples of every complex in ONE packed pass, reduced on the device.  On
        complexes with obstacle atoms the decoys of a group share the group's obstacles, and the clash that
        ranks them, the proximal stage and the recombination include the overlap with them.  ``batch``: a
        B = 1 batch, or a list of complexes (``batch.replicate_many``: group-major, complex g's decoys are segments
        g * n_decoys .. g * n_decoys + n_decoys - 1).  Decoy d of a complex with key k is sampled under the key
        ``batch.decoy_key(k, d)``: it is bit-equal to ``sampling(seed=seed)`` of that complex alone under that key, decoy 0 to what
        ``sampling(seed=seed)`` gives today.  With ``use_proximal`` every decoy then goes through the packed proximal stage and its
        accept rule, as ``sampling`` does for packed batches.  The per-residue clash at the final angles and
        ``Context.ensemble_reduce`` follow: ``select`` "clash" keeps the decoy with the lowest mean clash, "medoid" the one closest
        to the circular consensus, None decoy 0.

        Returns the selected angles [1, sum of the complexes' lengths, 4]; with ``return_all`` a dict: ``decoys`` = (angles
        [1, N, 4] of the packed batch, the packed batch), ``selected``, ``best`` [n_complexes] int32, ``dev`` / ``clash``
        [n_complexes * n_decoys] fp64, ``consensus`` / ``confidence`` [1, sum of lengths, 4] (circular mean; resultant length, 1 = all
        decoys agree) and ``keys`` (the decoys' noise keys, a list).

        ``recombine``: the decoys are then recombined per residue by clash descent, starting from the decoy
        ``select`` picks (None: decoy 0), at most ``recombine_sweeps`` sweeps; the returned angles are the recombined ones, and
        ``return_all`` keeps every key above as it is and adds ``recombined`` [1, sum of lengths, 4], ``pick`` int32 [sum of lengths]
        (the decoy every row was taken from), ``clash_trace`` fp64 [n_complexes, recombine_sweeps + 1], ``sweeps`` and ``converged``
        int32 [n_complexes].

        ``sasa``: ``return_all`` gains ``bsa``, fp64 [n_complexes * n_decoys]: the surface every decoy buries
        between its chains (``Context.sasa`` at the decoy's angles, ``seg_area[1] - seg_area[2]``).  Nothing else changes.

        ``polar``: ``return_all`` gains ``hbonds``, ``hbonds_interface`` and ``salt_interface``, int32
        [n_complexes * n_decoys] -- every decoy's hydrogen bonds, those between chains and its salt bridges between chains, from ONE
        ``Context.polar`` over the packed decoys -- and, with ``sasa`` too, ``buns_interface`` (buried unsatisfied polar atoms that
        the isolated chain exposes).  They rank nothing: ``select`` has no mode for them.

        ``clashscore``: ``return_all`` gains ``clashscore`` fp64 and ``clashes_interface`` int32
        [n_complexes * n_decoys] -- every decoy's all-atom clashscore with placed hydrogens and its serious overlaps between
        chains, from ONE ``Context.clashscore`` over the packed decoys.  Not MolProbity's number; ranking by it is untuned, so
        ``select`` has no mode for it.

        ``hbond_optimize``: ``return_all`` gains ``hnet_bonds`` and ``hnet_flips`` int64
        [n_complexes * n_decoys] -- the explicit-hydrogen bonds every decoy's movers make once its flips and rotatable hydrogens
        are optimised, and the rows flipped, from ONE ``Context.hbond_optimize`` over the packed decoys -- and, with ``clashscore``
        too, ``clashscore_hnet``: the score of the optimised structure with the rotatable hydrogens counted, beside the
        conventional one.  The decoys' angles are returned as sampled; nothing is ranked by these.

        ``refine_allatom``: behind the proximal stage, ONE ``Context.refine_allatom`` over the packed decoys
        lowers every decoy's explicit-hydrogen overlaps in chi space; everything after it (the ranking, the keys above) sees the
        refined angles, and ``return_all`` gains ``refine_moved`` int64 [n_complexes * n_decoys] (rows moved) and ``refine_F`` int64
        [n_complexes * n_decoys, 2] (the overlap energy before and after).  Nothing is ranked by them.

        ``guide``: every decoy is sampled with clash guidance, as ``sampling(guide=...)`` samples the complex
        alone under the decoy's key; None = today's path.  ``corrector``: likewise -- every decoy is a segment and gets
        its own corrector step size, the bits of ``sampling(seed=, corrector=)`` of that complex alone under ``decoy_key``."""
        from .batch import replicate, replicate_many
        if seed is None:
            raise ValueError("sample_ensemble needs seed: unseeded noise is laid out over the rows of the whole batch, so a decoy would "
                             "depend on its place in the packed batch; the seeded generator keys it by (seed, decoy key) alone")
        self._check_select(select)
        if isinstance(batch, (list, tuple)):
            packed = replicate_many(batch, n_decoys)
        else:
            if _get(batch, "seg_offsets") is not None or int(batch.num_proteins) != 1:
                raise ValueError("sample_ensemble takes a B = 1 batch or a list of complexes")
            packed = replicate(batch, n_decoys)
        if _get(packed, "fixed_mask") is not None:
            raise ValueError("ensembles under a fixed_mask are not supported: sample_ensemble samples every row")
        chi = self.sampling(packed, use_proximal=use_proximal, seed=seed, guide=guide, corrector=corrector)
        refine = None
        if refine_allatom:
            chi, refine = self._refine_tail(packed, chi)
        return self._reduce_ensemble(packed, chi, select, return_all, recombine, recombine_sweeps, sasa, polar, clashscore, hbond_optimize,
                                     refine)

    def repack_ensemble(self, batch, fixed_mask=None, *, n_decoys, seed, fixed_chi=None, fixed_mode="renoise",
                        use_proximal: bool = False, select="clash", return_all: bool = False, recombine: bool = False,
                        recombine_sweeps: int = 64, sasa: bool = False, guide=None, corrector=None, polar: bool = False,
                        clashscore: bool = False, hbond_optimize: bool = False, refine_allatom: bool = False):
        """``sample_ensemble`` under a pin: ``n_decoys`` seeded partial repackings of every complex in ONE packed
        pass, reduced on the device.  ``batch``: a B = 1 batch, or a list of complexes (per-complex data or B = 1 batches).  Every
        complex carries its ``fixed_mask`` (1 = keep; [1, L] on a B = 1 batch, [L] on per-complex data), or ``fixed_mask`` gives it:
        one mask for a B = 1 batch, a list of masks for a list.  ``fixed_chi`` likewise ([1, L, 4], or a list; default each
        complex's ``SC_D``).  The complexes are replicated with ``batch.replicate_many`` -- ``pack`` concatenates the masks --, the
        packed batch goes through ``repack`` (with ``use_proximal`` the pinned proximal stage, every decoy divided by its complex's
        unpacked size as the complex alone divides), then ``Context.clash`` and ``Context.ensemble_reduce``.

        Decoy d of a complex with key k has exactly the bits of ``repack`` of that complex alone under the key ``decoy_key(k, d)``,
        with and without ``use_proximal``.  pp_ensemble_reduce is used unchanged: kept rows are identical in every decoy, so their
        ``resultant`` is 1 to rounding and they add (to rounding) nothing to ``dev``; they enter the per-decoy means of ``dev`` and
        ``clash`` with the same weight in all decoys of a group, so they dilute both equally and do not change the ranking.
        Returns what ``sample_ensemble`` returns (``sasa``: the ``bsa`` key as there; ``polar``, ``clashscore``, ``hbond_optimize``, ``refine_allatom``: their keys as there; kept rows are not refined).  ``guide``,
        ``corrector``: as in ``sampling``."""
        from .batch import Batch, replicate_many
        self._check_select(select)
        single = not isinstance(batch, (list, tuple))
        if single and (_get(batch, "seg_offsets") is not None or int(batch.num_proteins) != 1):
            raise ValueError("repack_ensemble takes a B = 1 batch or a list of complexes")
        complexes = [batch] if single else list(batch)
        masks = [fixed_mask] if single else (list(fixed_mask) if fixed_mask is not None else [None] * len(complexes))
        refs = [fixed_chi] if single else (list(fixed_chi) if fixed_chi is not None else [None] * len(complexes))
        if len(masks) != len(complexes) or len(refs) != len(complexes):
            raise ValueError(f"{len(masks)} fixed masks / {len(refs)} fixed_chi for {len(complexes)} complexes")
        pinned, sizes = [], []
        for c, m in zip(complexes, masks):
            lead = c["residue_type"].dim() == 2
            n = int(c["residue_type"].shape[-1])
            m = _get(c, "fixed_mask") if m is None else m
            if m is None:
                raise ValueError("repack_ensemble needs a fixed_mask for every complex; sample_ensemble samples every row")
            m = torch.as_tensor(m).to(c["residue_type"].device) != 0
            if m.numel() != n:
                raise ValueError(f"fixed_mask has {m.numel()} elements, the complex has {n} rows")
            p = Batch(c)
            p["fixed_mask"] = m.reshape(1, n) if lead else m.reshape(n)
            pinned.append(p)
            sizes.append(n)
        packed = replicate_many(pinned, n_decoys)
        D = int(packed.n_decoys)
        ref = None
        if any(r is not None for r in refs):
            # the kept angles of every decoy, cut to the rows pack() kept: D copies per complex, in the order of the segments
            offs = packed.seg_offsets_host
            ref = torch.cat([torch.as_tensor(c["SC_D"] if r is None else r).to(device=packed.SC_D.device, dtype=torch.float32)
                             .reshape(-1, 4)[:offs[g * D + 1] - offs[g * D]]
                             for g, (c, r) in enumerate(zip(complexes, refs)) for _ in range(D)]).unsqueeze(0)
        chi = self.repack(packed, seed=seed, fixed_chi=ref, fixed_mode=fixed_mode, use_proximal=use_proximal,
                          norm_rows=[n for n in sizes for _ in range(D)] if use_proximal else None, guide=guide, corrector=corrector)
        refine = None
        if refine_allatom:
            chi, refine = self._refine_tail(packed, chi, packed.fixed_mask)
        return self._reduce_ensemble(packed, chi, select, return_all, recombine, recombine_sweeps, sasa, polar, clashscore, hbond_optimize,
                                     refine)

    def mutate(self, proteins_and_mutations, *, seed, radius=10.0, shell="ca", n_decoys=1, use_proximal: bool = False,
               select="clash", fixed_mode="renoise", max_rows=200_000, log=print, recombine: bool = False,
               recombine_sweeps: int = 64, sasa: bool = False, guide=None, corrector=None, polar: bool = False,
               clashscore: bool = False, hbond_optimize: bool = False, refine_allatom: bool = False):
        """Mutant modelling: put each mutation set into its complex, repack what it touches, return the mutant.
        ``proteins_and_mutations``: a list of ``(protein dict, mutations)`` pairs, ``mutations`` a string ("RA47A,EA48A") or dicts as
        ``featurize.parse_mutstr`` returns them; several sets of one protein are repeated pairs.  Set i of the call gets the noise
        key i unless its pair carries a third entry, the ``complex_key``.

        Per chunk of sets (packed so that ``n_decoys`` x rows <= ``max_rows``, as ``parallel.sample_sharded`` groups; a set shorter
        than 32 rows goes alone): ``featurize.mutant_model_data`` per set, one packed batch, one context, ONE ``Context.shell`` launch
        with seeds = ``mut_mask`` (``shell`` "ca": CA within ``radius`` of a mutated CA, PackPPI-AP's local subgraph; "atom": any
        atom within ``radius`` of an atom of a mutated residue, on the coordinates ``atom14`` builds at the batch's angles, the new
        side chains at chi = 0), ``fixed = ~shell`` on the device without a read-back, ``repack_ensemble``, and ``atom14`` of the
        selected decoy.

        A set's result does not depend on what it was packed with, and every row outside its shell keeps the wild type's ``SC_D``
        bit for bit.  Returns one dict per set: ``tag``, ``key``, ``SC_D`` [1, L, 4] (the selected decoy), ``X`` [1, L, 14, 3],
        ``shell`` bool [1, L], ``best`` (int32 scalar tensor), ``clash`` / ``dev`` fp64 [n_decoys], ``keys`` (the decoys' noise keys)
        and ``batch`` (the mutant B = 1 batch: residue types and atom mask of the mutant), tensors on the device.

        ``recombine``: ``SC_D`` and ``X`` are those of the decoys recombined per residue from the selected
        one, and every dict gains ``pick`` int32 [1, L] (the decoy each row was taken from; ``best`` outside the shell),
        ``clash_recombined`` (fp64 scalar tensor, on the scale of ``clash``) and ``rows_recombined`` (scalar tensor: rows with
        ``pick != best``).

        A protein dict with an ``obstacles`` entry (``pdb_io.obstacle_atoms``) gives its sets those fixed
        atoms: the clash every stage reports and optimises -- the pinned proximal stage, the ranking, the recombination -- includes
        the overlap with them.  The network and the shell rule do not see them.

        ``sasa``: every dict gains ``bsa`` fp64 [n_decoys], the surface each decoy buries between its chains.

        ``polar``: every dict gains ``hbonds``, ``hbonds_interface`` and ``salt_interface`` int32 [n_decoys]
        and, with ``sasa`` too, ``buns_interface`` [n_decoys], as ``sample_ensemble`` describes them.

        ``clashscore``: every dict gains ``clashscore`` fp64 and ``clashes_interface`` int32 [n_decoys], as
        ``sample_ensemble`` describes them.

        ``hbond_optimize``: every dict gains ``hnet_bonds`` and ``hnet_flips`` int64 [n_decoys] and, with
        ``clashscore`` too, ``clashscore_hnet`` fp64 [n_decoys], as ``sample_ensemble`` describes them.

        ``refine_allatom``: the shell rows of every decoy are refined against the explicit-hydrogen overlaps
        behind the pinned stage (rows outside the shell stay the wild type's, bit for bit); every dict gains ``refine_moved`` int64
        [n_decoys] and ``refine_F`` int64 [n_decoys, 2], and of the SELECTED decoy ``refine_steps`` int8 [rounds, 1, L, 4],
        ``refine_e`` int32 [1, L, 2], ``refine_chi0`` [1, L, 4] (its angles in front of the refinement) and ``refine_deltas`` (the
        step sizes in radians), gathered on the device.

        ``guide``: the shell is sampled with clash guidance, as in ``sampling``; rows outside the shell are
        fixed rows, which are never nudged.  ``corrector``: as in ``sampling``; the rows outside the shell
        are never moved and never counted."""
        from .batch import as_single, group_rows, pack, pad_rows, unpack
        from .featurize import mutant_model_data, parse_mutstr
        from .functional import _ctx_for
        from .lib import SHELL_MODES
        if shell not in SHELL_MODES:
            raise ValueError(f"shell must be one of {sorted(SHELL_MODES)}")
        n_decoys = int(n_decoys)
        if n_decoys < 1:
            raise ValueError(f"n_decoys must be at least 1, got {n_decoys}")
        sets, alone = [], []
        for i, pair in enumerate(proteins_and_mutations):
            protein, muts = pair[0], pair[1]
            key = int(pair[2]) if len(pair) > 2 and pair[2] is not None else i
            data = mutant_model_data(protein, parse_mutstr(muts) if isinstance(muts, str) else muts, log=log,
                                     obstacles=protein.get("obstacles"))
            n = int(data["num_nodes"])
            alone.append(n < 32 or int((data["residue_mask"] > 0).sum()) < 32)            # host tensors: no device read-back
            b = as_single(data).to(self.device)
            b["complex_key"] = key
            sets.append(b)
        results = [None] * len(sets)
        for grp in group_rows([int(b["max_size"]) for b in sets], alone, max_rows, n_decoys):
            members = [sets[i] for i in grp]
            pb = pack(members)
            gctx = _ctx_for(pb)
            xyz = gctx.atom14(pb.SC_D) if shell == "atom" else None
            sh = gctx.shell(pb.mut_mask, radius=radius, mode=shell, xyz=xyz)              # bool [1, N], stays on the device
            pinned = []
            for b, part in zip(members, unpack(pb, ~sh)):
                p = type(b)(b)
                p["fixed_mask"] = pad_rows(part, int(b["max_size"]), True)      # trailing rows pack() dropped keep their (zero) angles
                pinned.append(p)
            keep, self.keep_refine_report = getattr(self, "keep_refine_report", False), refine_allatom or getattr(self, "keep_refine_report", False)
            out = self.repack_ensemble(pinned, n_decoys=n_decoys, seed=seed, fixed_mode=fixed_mode, use_proximal=use_proximal,
                                       select=select, return_all=True, recombine=recombine, recombine_sweeps=recombine_sweeps,
                                       sasa=sasa, guide=guide, corrector=corrector, polar=polar, clashscore=clashscore,
                                       hbond_optimize=hbond_optimize, refine_allatom=refine_allatom)
            self.keep_refine_report = keep
            rep = None
            if refine_allatom:
                rep = self.refine_reports[-1] if keep else self.refine_reports.pop()
                seg_first = torch.tensor(out["decoys"][1].seg_offsets_host[:-1], device=self.device)
            final = out["recombined"] if recombine else out["selected"]
            pos = gctx.atom14(final)
            picks = unpack(pb, out["pick"].reshape(1, -1)) if recombine else [None] * len(members)
            parts = zip(grp, members, unpack(pb, final), unpack(pb, pos), unpack(pb, sh))
            for g, (i, b, chi, x, s) in enumerate(parts):
                n = int(b["max_size"])
                chi, x, s = pad_rows(chi, n, b["SC_D"]), pad_rows(x, n, b["X"]), pad_rows(s, n, False)
                results[i] = dict(tag=b["mutation_tag"], key=int(b["complex_key"]), SC_D=chi, X=x, shell=s, best=out["best"][g],
                                  clash=out["clash"][g * n_decoys:(g + 1) * n_decoys], dev=out["dev"][g * n_decoys:(g + 1) * n_decoys],
                                  keys=out["keys"][g * n_decoys:(g + 1) * n_decoys], batch=b)
                if recombine:
                    pk = picks[g]
                    moved = (pk != out["best"][g]).sum()
                    results[i].update(pick=pad_rows(pk, n, out["best"][g].expand(1, n)), clash_recombined=out["clash_trace"][g, -1], rows_recombined=moved)
                if sasa:
                    results[i]["bsa"] = out["bsa"][g * n_decoys:(g + 1) * n_decoys]
                for k in ("hbonds", "hbonds_interface", "salt_interface", "buns_interface") if polar else ():
                    if k in out:
                        results[i][k] = out[k][g * n_decoys:(g + 1) * n_decoys]
                for k in ("clashscore", "clashes_interface") if clashscore else ():
                    results[i][k] = out[k][g * n_decoys:(g + 1) * n_decoys]
                for k in ("hnet_bonds", "hnet_flips", "clashscore_hnet") if hbond_optimize else ():
                    if k in out:
                        results[i][k] = out[k][g * n_decoys:(g + 1) * n_decoys]
                for k in ("refine_moved", "refine_F") if refine_allatom else ():
                    results[i][k] = out[k][g * n_decoys:(g + 1) * n_decoys]
                if rep is not None:
                    # the rows of the selected decoy in the packed call, taken on the device; rows pack() dropped took no step
                    offs = out["decoys"][1].seg_offsets_host
                    ln = offs[g * n_decoys + 1] - offs[g * n_decoys]
                    rows = seg_first[g * n_decoys + out["best"][g].long()] + torch.arange(ln, device=self.device)
                    R = rep.steps.shape[0]
                    st, en = rep.steps.reshape(R, 1, -1, 4)[:, :, rows], rep.e.reshape(1, -1, 2)[:, rows]
                    results[i].update(refine_steps=torch.cat([st, st.new_zeros(R, 1, n - ln, 4)], 2), refine_e=torch.cat([en, en.new_zeros(1, n - ln, 2)], 1),
                                      refine_chi0=pad_rows(rep.chi0.reshape(1, -1, 4)[:, rows], n, b["SC_D"]), refine_deltas=rep.deltas)
        return results

    def sample_from(self, batch, SC_D_init, sde_noise=None):
        """The reverse-diffusion loop of ``sampling`` from given initial noised angles (parity runs inject the reference's
        own draw; the packed multi-complex path injects per-complex draws)."""
        return self._context(batch).sample(SC_D_init, self.schedule, self.hparams.sample_cfg.mode, sde_noise)

    def saturated(self) -> int:
        """Sticky flag word of the context of the last batch (0 = clean; see lib.Context.saturated).  Bits 0 / 1: a hidden
        activation reached the f16 maximum (results are not fp32-equivalent for this checkpoint); bit 2: a NaN / infinity entered
        with the batch or the angles (the reference would return NaN)."""
        return self._ctx.saturated() if self._ctx is not None else 0

    def compute_rmsd(self, true_coords, pred_coords, atom_mask, residue_mask):
        w = atom_mask * residue_mask[..., None]
        return (torch.sum((true_coords - pred_coords) ** 2, dim=-1) * w).sum() / (w + self.eps).sum()

    def analyze_samples(self, batch, SC_D_sample=None):
        true, m, pi1 = batch["SC_D"], batch["SC_D_mask"], batch["chi_1pi_periodic_mask"]
        metric = {}
        for i in range(self.NUM_CHI_ANGLES):
            n = m[..., i].sum()
            n = n if n != 0 else 1
            diff = (SC_D_sample[..., i] - true[..., i]).abs()
            acc = torch.logical_and(diff * 180 / np.pi < 20, diff > 0).float()
            ae = torch.minimum(diff, 2 * np.pi - diff)
            ae = torch.where(pi1[..., i], torch.minimum(ae, np.pi - ae), ae)
            metric[f"chi_{i}_ae_rad"] = ae.sum() / n
            metric[f"chi_{i}_ae_deg"] = (ae * 180 / np.pi).sum() / n
            metric[f"chi_{i}_acc"] = acc.sum() / n
        pred = self._geometry_context(batch).atom14(SC_D_sample)
        metric["atom_rmsd"] = self.compute_rmsd(batch.X, pred, batch.atom_mask, batch.residue_mask)
        return metric

    def get_atom14_coords(self, batch, SC_D):
        return self._geometry_context(batch).atom14(SC_D)
