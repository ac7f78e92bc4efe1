"""Weight contract of the PackPPI-MSC score network (112 tensors, 1 439 172 fp32 params).

Key names and ``nn.Linear`` ``[out, in]`` layouts are those of the reference Lightning
checkpoint's ``state_dict`` (TorsionalDiffusion.py:39-68, encoder.py:82-85,
layers.py:11-18,36-63); SURVEY.md §8b.
"""
from collections import OrderedDict

import numpy as np
import torch

H = 128          # node / edge / hidden width
NODE_IN = 51     # one-hot(21) + bb sincos(6) + sc sincos(8) + t-emb(16)
EDGE_IN = 468    # relpos(65) + 25*16 rbf + chain flag + 2 dihedrals
MSG_IN = 456     # h_V_i | h_E_ij | h_V_j | 72 geometric features
N_POINTS = 8
N_LAYERS = 3


def weight_spec():
    """Ordered (name, shape) list of every tensor the sampler reads."""
    s = []

    def lin(name, o, i):
        s.append((name + ".weight", (o, i)))
        s.append((name + ".bias", (o,)))

    def ln(name):
        s.append((name + ".weight", (H,)))
        s.append((name + ".bias", (H,)))

    lin("encoder.node_embedding", H, NODE_IN)
    ln("encoder.norm_nodes")
    lin("encoder.edge_embedding", H, EDGE_IN)
    ln("encoder.norm_edges")
    for l in range(N_LAYERS):
        p = f"mpnn.mpnn_layers.{l}."
        lin(p + "points_fn_node", 3 * N_POINTS, H)
        lin(p + "points_fn_edge", 3 * N_POINTS, H)
        for fn in ("node_message_fn", "edge_message_fn"):
            lin(p + fn + ".W_in", H, MSG_IN)
            lin(p + fn + ".W_inter.0", H, H)
            lin(p + fn + ".W_out", H, H)
        for k in range(4):
            ln(p + f"norm.{k}")
        for fn in ("node_dense", "edge_dense"):
            lin(p + fn + ".W_in", 4 * H, H)
            lin(p + fn + ".W_out", H, 4 * H)
    lin("decoder_score.0.W_in", H // 2, H)
    lin("decoder_score.0.W_out", H // 4, H // 2)
    lin("decoder_score.2.W_in", H // 8, H // 4)
    lin("decoder_score.2.W_out", 4, H // 8)
    return s


def make_random_state_dict(seed: int = 0) -> "OrderedDict[str, torch.Tensor]":
    """Seeded stand-in weights (the trained checkpoint is not distributed with the reference).

    Matrices: xavier-uniform (as TorsionalDiffusion.py:80-82 initialises them); biases
    N(0, 0.1); LayerNorm gains 1 + N(0, 0.1).  Drawn from a CPU ``torch.Generator`` in
    spec order, so every machine with this torch build gets identical values.
    """
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    sd = OrderedDict()
    for name, shape in weight_spec():
        if len(shape) == 2:
            bound = float(np.sqrt(6.0 / (shape[0] + shape[1])))
            w = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        elif ".norm" in name and name.endswith("weight") or "norm_" in name and name.endswith("weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
        else:
            w = 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
        sd[name] = w
    return sd


def check_state_dict(sd, strict: bool = False):
    """Validate names/shapes; returns an OrderedDict of contiguous fp32 CPU tensors in spec order.

    ``strict=False`` mirrors ``load_from_checkpoint(strict=False)`` (eval_diffusion.py:33-40)
    for *extra* keys; every tensor the sampler reads must still be present.
    """
    out = OrderedDict()
    for name, shape in weight_spec():
        if name not in sd:
            raise RuntimeError(f"checkpoint is missing weight '{name}'")
        t = torch.as_tensor(sd[name]).detach().to(torch.float32).cpu().contiguous()
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"weight '{name}' has shape {tuple(t.shape)}, expected {shape}")
        out[name] = t
    if strict:
        extra = set(sd.keys()) - set(out.keys())
        if extra:
            raise RuntimeError(f"unexpected keys in state_dict: {sorted(extra)[:5]}")
    return out


# ---- PackPPI-AP (AffinityPrediction.py:22-98) ------------------------------------------------------------------------------
AP_NODE_IN = 35          # mutation_encoder: time_embedding_dim = 0, so node_in without the 16 time-embedding inputs
AFFINITY_MODES = ("network", "linear", "esm")


def affinity_head_spec(mode: str = "network"):
    """Ordered (name, shape) list of the tensors AffinityPrediction owns besides the two networks: in ``network`` mode
    ``mut_bias`` (:73-77), ``seq_embedding`` (:79), ``mutation_fusion.{0,2}`` (:81-88); in every mode ``ddg_predictor``
    (:90-94).  The order is the one pp_affinity_create reads."""
    s = []
    if mode == "network":
        s += [("mut_bias.weight", (2, H)), ("seq_embedding.weight", (21, H)),
              ("mutation_fusion.0.weight", (H, 3 * H)), ("mutation_fusion.0.bias", (H,)),
              ("mutation_fusion.2.weight", (H, H)), ("mutation_fusion.2.bias", (H,))]
    s += [("ddg_predictor.0.weight", (H, H)), ("ddg_predictor.0.bias", (H,)),
          ("ddg_predictor.2.weight", (H, H)), ("ddg_predictor.2.bias", (H,)),
          ("ddg_predictor.4.weight", (1, H)), ("ddg_predictor.4.bias", (1,))]
    return s


def mutation_branch_spec():
    """(AP key, score-network key, shape) of the mutation encoder + MPNN (AffinityPrediction.py:50-71): the score network's
    encoder / mpnn tensors, except that the node embedding has 35 input columns (no time embedding) and there is no
    decoder."""
    out = []
    for name, shape in weight_spec():
        if name.startswith("decoder_score."):
            continue
        if name.startswith("encoder."):
            ap = "mutation_encoder." + name[len("encoder."):]
        else:
            ap = "mutation_mpnn." + name[len("mpnn."):]
        if name == "encoder.node_embedding.weight":
            shape = (H, AP_NODE_IN)
        out.append((ap, name, shape))
    return out


def affinity_weight_spec(mode: str = "network"):
    """Ordered (name, shape) list of every tensor of an AffinityPrediction checkpoint's ``state_dict`` in ``mode``: the
    frozen pretrained network under ``pret.`` and the tensors of affinity_head_spec / mutation_branch_spec."""
    if mode not in ("network", "linear"):
        raise NotImplementedError(f"AffinityPrediction mode '{mode}' (esm needs ESM-2 representations) is not supported")
    s = [("pret." + n, shp) for n, shp in weight_spec()]
    if mode == "network":
        s += [(ap, shp) for ap, _, shp in mutation_branch_spec()]
    return s + affinity_head_spec(mode)


def make_random_affinity_state_dict(seed: int = 0, mode: str = "network") -> "OrderedDict[str, torch.Tensor]":
    """Seeded stand-in weights for the tensors AffinityPrediction owns (no ``pret.`` keys: the pretrained network comes from
    ``make_random_state_dict``).  Same rules as there; embedding tables N(0, 0.1), the ``mut_bias`` padding row included (the
    reference reads whatever value row 0 holds)."""
    g = torch.Generator(device="cpu").manual_seed(int(seed))
    sd = OrderedDict()
    names = [(n, shp) for n, shp in affinity_weight_spec(mode) if not n.startswith("pret.")]
    for name, shape in names:
        if len(shape) == 2 and name not in ("seq_embedding.weight", "mut_bias.weight"):
            bound = float(np.sqrt(6.0 / (shape[0] + shape[1])))
            w = (torch.rand(shape, generator=g, dtype=torch.float32) * 2 - 1) * bound
        elif ("norm" in name) and name.endswith("weight"):
            w = 1.0 + 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
        else:
            w = 0.1 * torch.randn(shape, generator=g, dtype=torch.float32)
        sd[name] = w
    return sd


def check_affinity_state_dict(sd, mode: str = "network"):
    """Every tensor of affinity_weight_spec(mode) except the ``pret.`` ones, validated as check_state_dict does: a missing
    key or a wrong shape raises RuntimeError naming it.  Returns an OrderedDict of contiguous fp32 CPU tensors."""
    out = OrderedDict()
    for name, shape in affinity_weight_spec(mode):
        if name.startswith("pret."):
            continue
        if name not in sd:
            raise RuntimeError(f"affinity checkpoint is missing weight '{name}'")
        t = torch.as_tensor(sd[name]).detach().to(torch.float32).cpu().contiguous()
        if tuple(t.shape) != tuple(shape):
            raise RuntimeError(f"weight '{name}' has shape {tuple(t.shape)}, expected {shape}")
        out[name] = t
    return out


def mutation_branch_state_dict(sd) -> "OrderedDict[str, torch.Tensor]":
    """The mutation encoder + MPNN as a score-network state_dict (weight_spec order) for pp_plan_create: node-embedding
    columns 35..50 (the time embedding this encoder does not have) and the decoder are zero.  Zero columns times the time
    embedding add exact zeros; the decoder's output is not read."""
    ap = {score: ap for ap, score, _ in mutation_branch_spec()}
    out = OrderedDict()
    for name, shape in weight_spec():
        if name in ap:
            t = torch.as_tensor(sd[ap[name]]).detach().to(torch.float32).cpu()
            if name == "encoder.node_embedding.weight":
                t = torch.cat([t, torch.zeros(H, NODE_IN - AP_NODE_IN)], 1)
            out[name] = t.contiguous()
        else:
            out[name] = torch.zeros(shape, dtype=torch.float32)
    return out
