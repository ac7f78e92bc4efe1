"""``AffinityPrediction``: PackPPI-AP, the binding ddG predictor (src/models/AffinityPrediction.py), on the HIP path.

Inference surface of the reference Lightning module: ``load_from_checkpoint(ckpt, pre_checkpoint_path=...)`` (eval_affinity.py:
27-38), ``get_pret_feature`` (:109-122), ``get_local_subgraph`` (:124-145), ``encode`` (:148-169) and ``forward`` (:171-194).
Modes ``network`` and ``linear``; ``esm`` needs ESM-2 representations and raises NotImplementedError.  Training is out of
scope.  ``predict_many`` evaluates many mutation sets at once: one packed context per branch (a SKEMPI table or a mutational
scan), each set with exactly the bits of its own ``forward``.

Where the work runs: the pretrained network at t = 0 is ``pp_score`` (the h_V it returns); the mutation encoder + MPNN are
a second plan of the score-network kernels (weights.mutation_branch_state_dict) on a context whose residue_mask is the
local mask; ``k_affinity_embed`` does what lies between the two networks and ``k_affinity_head`` the max over residues and
ddg_predictor (csrc/pp_node.hip, csrc/pp_affinity.hip).  Only the local mask is computed on the host, with torch.cdist on a
CPU copy of the CA coordinates, which is the reference CPU path exactly; ``predict_many(local_mask="device")`` takes the masks
of all sets from one pp_ctx_shell launch instead.
"""
from typing import Any, Dict, List, Optional

import torch

from .batch import Batch, MUT_KEYS, pack
from .lib import AffinityHead, Context, Plan
from .module import _TolerantPickle, read_checkpoint_state_dict
from .weights import AFFINITY_MODES, check_affinity_state_dict, check_state_dict, mutation_branch_state_dict

# the keys AffinityPrediction.forward swaps for their `_mut` copies to make the mutant batch (:178-181)
SWAP_KEYS = ("atom_mask", "residue_type", "SC_D", "SC_D_sincos", "SC_D_mask", "chi_1pi_periodic_mask",
             "chi_2pi_periodic_mask")


def read_checkpoint(path, map_location="cpu") -> Dict[str, Any]:
    """The whole Lightning checkpoint dict (state_dict + hyper_parameters), readable without Lightning / OmegaConf."""
    try:
        return torch.load(path, map_location=map_location, weights_only=True)
    except Exception:
        return torch.load(path, map_location=map_location, weights_only=False, pickle_module=_TolerantPickle)


def mutant_view(batch) -> Batch:
    """``batch_mt`` of AffinityPrediction.forward: a shallow copy with the SWAP_KEYS taken from their ``_mut`` keys."""
    mt = Batch(batch)
    for k in SWAP_KEYS:
        mt[k] = batch[k + "_mut"]
    return mt


class AffinityPrediction:
    def __init__(self, state_dict: Dict[str, torch.Tensor], pret_state_dict: Dict[str, torch.Tensor], mode: str = "network",
                 device="cuda", encoder_cfg: Any = None, model_cfg: Any = None):
        """``state_dict``: AffinityPrediction's own tensors (weights.affinity_head_spec + mutation_branch_spec; a missing one
        raises RuntimeError naming it); ``pret_state_dict``: the pretrained score network (weights.weight_spec)."""
        from .config import check_compiled_dims
        if mode not in AFFINITY_MODES:
            raise ValueError(f"Invalid mode '{mode}'. Valid modes are: {list(AFFINITY_MODES)}.")
        if mode == "esm":
            raise NotImplementedError("AffinityPrediction mode 'esm' needs ESM-2 representations and is not supported")
        check_compiled_dims(encoder_cfg, model_cfg)
        self.hparams = type("HParams", (), {})()
        self.hparams.mode = mode
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError(f"packppi_amd.AffinityPrediction runs on the MI355X HIP device only (got device '{device}')")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        own = check_affinity_state_dict(state_dict, mode)
        self.pret_plan = Plan(check_state_dict(pret_state_dict), self.device)
        self.mutation_plan = Plan(mutation_branch_state_dict(own), self.device) if mode == "network" else None
        self.head = AffinityHead(own, self.device, mode)
        self._contexts: List[Context] = []

    # ---- construction ----------------------------------------------------------------------
    @classmethod
    def load_from_checkpoint(cls, checkpoint_path, pre_checkpoint_path=None, map_location=None, strict=False, mode=None,
                             **kwargs):
        """As eval_affinity.py:27-38: ``mode`` defaults to the checkpoint's hyper_parameters, the pretrained network comes from
        ``pre_checkpoint_path`` (default: the one in hyper_parameters) and, as with the reference's strict=False load, the
        checkpoint's own ``pret.*`` tensors override it."""
        ckpt = read_checkpoint(checkpoint_path)
        sd = ckpt["state_dict"] if isinstance(ckpt, dict) and "state_dict" in ckpt else ckpt
        sd = {k: v for k, v in sd.items() if isinstance(v, torch.Tensor)}
        hp = ckpt.get("hyper_parameters", {}) if isinstance(ckpt, dict) else {}
        hp = hp if isinstance(hp, dict) else {}
        mode = mode or hp.get("mode") or "network"
        pre = pre_checkpoint_path or hp.get("pre_checkpoint_path")
        pret = dict(read_checkpoint_state_dict(pre)) if pre else {}
        pret.update({k[len("pret."):]: v for k, v in sd.items() if k.startswith("pret.")})
        return cls(sd, pret, mode=mode, device=map_location or "cuda", **kwargs)

    def eval(self):
        return self

    def set_mutation_knn_ties(self, mode: str):
        """Tie convention of the mutation branch's neighbour search (lib.Plan.set_knn_ties); its outputs do not depend on
        it: the tied rows are the ones outside the local mask, and their edges are masked."""
        self.mutation_plan.set_knn_ties(mode)

    def saturated(self) -> int:
        """OR of the sticky flag words (lib.Context.saturated) of the contexts of the last forward / predict_many."""
        out = 0
        for c in self._contexts:
            out |= c.saturated()
        return out

    # ---- reference surface -------------------------------------------------------------------
    @torch.no_grad()
    def get_pret_feature(self, batch):
        """h_V of the pretrained network at t = 0 on the batch's own angles [B, L, 128]."""
        ctx = Context(self.pret_plan, batch)
        self._contexts.append(ctx)
        return ctx.score(batch["SC_D"], 0.0)[1]

    @staticmethod
    def get_local_subgraph(X, mut_mask, radius=10):
        """Residues whose CA lies within `radius` of a mutated residue's CA [B, L] float32 (not multiplied by residue_mask,
        as the reference).  torch.cdist on CPU copies: the reference CPU path, exactly."""
        Xc = X.detach().float().cpu()
        mm = mut_mask.detach().cpu()
        B, L, _ = Xc.shape
        dist = torch.cdist(Xc.view(B, L, -1), Xc.view(B, L, -1))
        local = (dist < radius) & mm.unsqueeze(1).expand(B, L, L).to(torch.uint8)
        return local.any(dim=2).to(torch.float32).to(X.device)

    def _mutation_context(self, batch, local_mask):
        mb = Batch(batch)
        mb["residue_mask"] = local_mask.to(device=self.device, dtype=torch.float32).reshape(batch["residue_mask"].shape)
        ctx = Context(self.mutation_plan, mb)
        self._contexts.append(ctx)
        return ctx

    @torch.no_grad()
    def encode(self, batch, h_pret=None, ctx=None):
        """The mutation branch's h [B, L, 128] (exact zeros outside the local mask)."""
        if ctx is None:
            ctx = self._mutation_context(batch, self.get_local_subgraph(batch["X"][:, :, 1, :], batch["mut_mask"]))
        if h_pret is None:
            h_pret = self.get_pret_feature(batch)
        return self.head.encode(ctx, batch["residue_type"], batch["SC_D_sincos"], batch["mut_mask"], h_pret)

    def _features(self, batch):
        self._contexts = []
        mt = mutant_view(batch)
        p_wt, p_mt = self.get_pret_feature(batch), self.get_pret_feature(mt)
        if self.hparams.mode != "network":
            return p_wt, p_mt
        ctx = self._mutation_context(batch, self.get_local_subgraph(batch["X"][:, :, 1, :], batch["mut_mask"]))
        return self.encode(batch, p_wt, ctx), self.encode(mt, p_mt, ctx)

    @torch.no_grad()
    def forward(self, batch):
        """(loss, ddg_pred [B, 1]) of AffinityPrediction.forward; the max over residues sees every row of the padded batch."""
        h_wt, h_mt = self._features(batch)
        B, L = batch["residue_type"].shape
        ddg, inv = self.head.predict(h_wt, h_mt, [b * L for b in range(B + 1)])
        self.last_ddg_inv = inv.reshape(B, 1)
        labels = batch["ddg"].to(self.device).reshape(-1)
        loss = (torch.mean((ddg - labels) ** 2) + torch.mean((inv + labels) ** 2)) / 2
        return loss, ddg.reshape(B, 1)

    __call__ = forward

    @torch.no_grad()
    def predict_many(self, batches, local_mask="host"):
        """ddg and ddg_inv [n] of n mutation sets (``featurize.mutant_data`` outputs or B = 1 batches): one packed context
        per branch.  Every row of every set is kept (batch.pack(trim=False)); each set gets the bits of its own forward.
        ``local_mask``: "host" (default, the pinned reference path: ``get_local_subgraph`` once per set, torch.cdist on CPU copies)
        or "device": the local masks of all sets come from ONE ``Context.shell(mode="ca", radius=10)`` launch on the wild-type
        context of the pretrained network (pp_ctx_shell) -- no copy of the coordinates to the host.  The two
        agree wherever no CA pair lies within rounding of the radius; mode ``linear`` has no local mask and ignores the switch."""
        if local_mask not in ("host", "device"):
            raise ValueError("local_mask must be 'host' or 'device'")
        batches = list(batches)
        wt = pack(batches, trim=False).to(self.device)
        missing = [k for k in MUT_KEYS if k not in wt]
        if missing:
            raise RuntimeError(f"predict_many needs mutation batches (missing {missing})")
        offs = wt["seg_offsets_host"]
        h_wt, h_mt = self._features(wt) if self.hparams.mode != "network" else self._packed_network(batches, wt, local_mask)
        ddg, inv = self.head.predict(h_wt, h_mt, offs)
        return ddg, inv

    def _packed_network(self, batches, wt, local_mask="host"):
        self._contexts = []
        mt = mutant_view(wt)
        p_wt, p_mt = self.get_pret_feature(wt), self.get_pret_feature(mt)
        if local_mask == "device":
            # the wild-type context get_pret_feature just made: its segment table keeps every set's shell inside the set
            ctx = self._mutation_context(wt, self._contexts[0].shell(wt["mut_mask"], radius=10.0, mode="ca"))
            return self.encode(wt, p_wt, ctx), self.encode(mt, p_mt, ctx)
        local = []
        for b in batches:
            X = b["X"] if b["X"].dim() == 4 else b["X"].unsqueeze(0)
            m = b["mut_mask"] if b["mut_mask"].dim() == 2 else b["mut_mask"].unsqueeze(0)
            local.append(self.get_local_subgraph(X[:, :, 1, :], m).reshape(-1))
        ctx = self._mutation_context(wt, torch.cat(local).unsqueeze(0))
        return self.encode(wt, p_wt, ctx), self.encode(mt, p_mt, ctx)
