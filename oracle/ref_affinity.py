"""CPU oracle for PackPPI-AP, the binding ddG predictor (src/models/AffinityPrediction.py).  TEST INFRASTRUCTURE ONLY.

A from-the-spec restatement in plain torch of what the HIP path of ``packppi_amd/affinity.py`` must reproduce, under the rules
of ``oracle/ref_cpu.py``: imported only by ``tests/``, never by the product path under ``packppi_amd/``.  The dtype follows the
inputs: a ``.double()`` batch with ``.double()`` weights (``to_double``) gives the fp64 arbiter.

Parity status: PINNED.  ``tests/test_affinity_oracle.py`` checks every function here against the tensors the unmodified
reference wrote into ``tests/golden/g11_affinity_*.npz`` (``tools/oracle/make_golden_affinity.py``).

The two networks (the pretrained score network and the mutation encoder + MPNN) are ``ref_cpu``'s; the mutation branch's
tensors are read under their score-network names (``branch_state_dict``).  Each function cites the reference lines (relative
to the upstream repo root) it follows.
"""
import torch
import torch.nn.functional as F

from . import ref_cpu as O

# the keys AffinityPrediction.forward swaps for their `_mut` copies to make the mutant batch (AffinityPrediction.py:177-180)
SWAP_KEYS = ("atom_mask", "residue_type", "SC_D", "SC_D_sincos", "SC_D_mask", "chi_1pi_periodic_mask",
             "chi_2pi_periodic_mask")


def to_double(x):
    """A batch or a state_dict with every float32 tensor in float64 (the fp64 arbiter's inputs); the rest as it is."""
    return type(x)((k, (v.double() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v)) for k, v in x.items())


def mutant_view(batch):
    """``batch_mt`` of AffinityPrediction.forward (:177-180): a shallow copy with the SWAP_KEYS taken from ``<key>_mut``."""
    mt = type(batch)(batch)
    for k in SWAP_KEYS:
        mt[k] = batch[k + "_mut"]
    return mt


def branch_state_dict(ap_sd):
    """``mutation_encoder.*`` / ``mutation_mpnn.*`` (:50-71) under the names ``ref_cpu`` reads: ``encoder.*`` / ``mpnn.*``.
    The node embedding keeps its 35 input columns (time_embedding_dim = 0, :55)."""
    out = {}
    for k, v in ap_sd.items():
        if k.startswith("mutation_encoder."):
            out["encoder." + k[len("mutation_encoder."):]] = v
        elif k.startswith("mutation_mpnn."):
            out["mpnn." + k[len("mutation_mpnn."):]] = v
    return out


def static_from_graph(sd, batch, E_idx, zero_self_dihedral=False):
    """``ref_cpu.encode_static`` on given neighbour lists: (E_idx, h_E0) (encoder.py:205-215,231-244)."""
    E = O.edge_features(batch["X"], E_idx, batch["residue_index"], batch["chain_indices"], zero_self_dihedral)
    h_E = O._ln(O._linear(E, sd["encoder.edge_embedding.weight"], sd["encoder.edge_embedding.bias"]),
                sd["encoder.norm_edges.weight"], sd["encoder.norm_edges.bias"])
    return E_idx, h_E


def _static(sd, batch, static, zero_self_dihedral):
    """None: the oracle's own search; an int64 tensor: neighbour lists to use; a pair: (E_idx, h_E0) as it is."""
    if static is None:
        return O.encode_static(sd, batch, zero_self_dihedral)
    if isinstance(static, torch.Tensor):
        return static_from_graph(sd, batch, static, zero_self_dihedral)
    return static


def pret_feature(pret_sd, batch, static=None, zero_self_dihedral=False):
    """h_V [B,L,128] of the pretrained network at t = 0 on the batch's own angles (AffinityPrediction.py:108-122)."""
    B, L = batch["residue_type"].shape
    t = torch.zeros(B * L, dtype=batch["X"].dtype)
    return O.network(pret_sd, batch, batch["SC_D"], t, _static(pret_sd, batch, static, zero_self_dihedral), zero_self_dihedral)[1]


def local_subgraph(X_ca, mut_mask, radius=10):
    """Residues whose CA lies within ``radius`` of a mutated residue's CA, [B,L] float32 (AffinityPrediction.py:124-145).
    Not multiplied by residue_mask.  The distances are taken in float32 whatever the input's dtype: the mask is a discrete
    input of everything after it, and the fp64 arbiter must run on the subgraph the reference selects."""
    B, L, _ = X_ca.shape
    Xf = X_ca.float().reshape(B, L, -1)
    near = torch.cdist(Xf, Xf) < radius
    mm = mut_mask.unsqueeze(1).expand(B, L, L).to(torch.uint8)
    return (near & mm).any(dim=2).to(torch.float32)


def encode(ap_sd, batch, h_pret, local_mask, static=None, zero_self_dihedral=False):
    """AffinityPrediction.encode after the pretrained features (:148-169): h [B,L,128], zero outside ``local_mask``.

    mutation_encoder (encoder.py:198-246 with mask = local_mask and no time embedding): Linear(35,128) + LayerNorm on
    [one-hot(S) | BB_D_sincos | SC_D_sincos AS GIVEN]; fusion MLP on [h_pret | that | seq_embedding(S)] plus
    mut_bias[mut_mask] (:162-166); mutation_mpnn (mpnn.py:47-62) with mask = local_mask."""
    sd = branch_state_dict(ap_sd)
    dt = batch["X"].dtype
    B, L = batch["residue_type"].shape
    S = batch["residue_type"]
    mask = local_mask.to(dt).reshape(B, L)
    mb = type(batch)(batch)
    mb["residue_mask"] = mask
    E_idx, h_E = _static(sd, mb, static, zero_self_dihedral)
    V = torch.cat([F.one_hot(S, 21).to(dt), batch["BB_D_sincos"].reshape(B, L, 6), batch["SC_D_sincos"].reshape(B, L, 8)], -1)
    h_mut = O._ln(O._linear(V, sd["encoder.node_embedding.weight"], sd["encoder.node_embedding.bias"]),
                  sd["encoder.norm_nodes.weight"], sd["encoder.norm_nodes.bias"])
    x = torch.cat([h_pret, h_mut, ap_sd["seq_embedding.weight"][S]], -1)
    x = F.relu(O._linear(x, ap_sd["mutation_fusion.0.weight"], ap_sd["mutation_fusion.0.bias"]))
    h_V = O._linear(x, ap_sd["mutation_fusion.2.weight"], ap_sd["mutation_fusion.2.bias"])
    h_V = h_V + ap_sd["mut_bias.weight"][batch["mut_mask"].long()]
    R, tr = O.backbone_frames(batch["X"])
    mask_att = mask[..., None] * O._gather_nodes(mask[..., None], E_idx)[..., 0]
    for l in range(3):
        # the last layer's edge update feeds nothing (mpnn.py:62 returns h_V only)
        h_V, h_E = O.ipmp_layer(sd, l, h_V, h_E, E_idx, R, tr, mask, mask_att, edge_update=(l < 2))
    return h_V


def ddg_predictor(ap_sd, x):
    """Linear ReLU Linear ReLU Linear(128, 1) (AffinityPrediction.py:90-94)."""
    x = F.relu(O._linear(x, ap_sd["ddg_predictor.0.weight"], ap_sd["ddg_predictor.0.bias"]))
    x = F.relu(O._linear(x, ap_sd["ddg_predictor.2.weight"], ap_sd["ddg_predictor.2.bias"]))
    return O._linear(x, ap_sd["ddg_predictor.4.weight"], ap_sd["ddg_predictor.4.bias"])


def pooled(h_wt, h_mt, seg_offsets):
    """Per segment the max over rows of h_mt - h_wt and of h_wt - h_mt, [n_seg,128] each (:189-190); rows are those of the
    flattened [rows,128] tensors, padding rows included; an empty segment gives -inf (the identity of max)."""
    hw, hm = h_wt.reshape(-1, h_wt.shape[-1]), h_mt.reshape(-1, h_mt.shape[-1])
    fwd, inv = [], []
    for a, b in zip(seg_offsets[:-1], seg_offsets[1:]):
        a, b = int(a), int(b)
        if b > a:
            fwd.append((hm[a:b] - hw[a:b]).max(dim=0)[0])
            inv.append((hw[a:b] - hm[a:b]).max(dim=0)[0])
        else:
            fwd.append(torch.full((hw.shape[-1],), float("-inf"), dtype=hw.dtype))
            inv.append(torch.full((hw.shape[-1],), float("-inf"), dtype=hw.dtype))
    return torch.stack(fwd), torch.stack(inv)


def head(ap_sd, h_wt, h_mt, seg_offsets):
    """(ddg [n_seg], ddg_inv [n_seg]) of AffinityPrediction.forward (:189-190) per segment of rows."""
    fwd, inv = pooled(h_wt, h_mt, seg_offsets)
    return ddg_predictor(ap_sd, fwd).reshape(-1), ddg_predictor(ap_sd, inv).reshape(-1)


def features(ap_sd, pret_sd, batch, mode, pret_static=None, mut_static=None, local_mask=None, zero_self_dihedral=False):
    """(h_wt, h_mt) of AffinityPrediction.forward (:177-187): the mutation branch's output in mode ``network``, the
    pretrained features in mode ``linear``.  The two statics serve the wild type and the mutant: the graph and the edge
    embedding depend on neither's side chains."""
    if mode not in ("network", "linear"):
        raise NotImplementedError(mode)
    mt = mutant_view(batch)
    pret_static = _static(pret_sd, batch, pret_static, zero_self_dihedral)
    p_wt = pret_feature(pret_sd, batch, pret_static, zero_self_dihedral)
    p_mt = pret_feature(pret_sd, mt, pret_static, zero_self_dihedral)
    if mode == "linear":
        return p_wt, p_mt
    if local_mask is None:
        local_mask = local_subgraph(batch["X"][:, :, 1, :], batch["mut_mask"])
    mb = type(batch)(batch)
    mb["residue_mask"] = local_mask.to(batch["X"].dtype)
    mut_static = _static(branch_state_dict(ap_sd), mb, mut_static, zero_self_dihedral)
    return (encode(ap_sd, batch, p_wt, local_mask, mut_static, zero_self_dihedral),
            encode(ap_sd, mt, p_mt, local_mask, mut_static, zero_self_dihedral))


def forward(ap_sd, pret_sd, batch, mode, pret_static=None, mut_static=None, local_mask=None, zero_self_dihedral=False):
    """(loss, ddg [B,1], ddg_inv [B,1]) of AffinityPrediction.forward (:171-194); the max sees every row of the padded batch."""
    h_wt, h_mt = features(ap_sd, pret_sd, batch, mode, pret_static, mut_static, local_mask, zero_self_dihedral)
    B, L = batch["residue_type"].shape
    ddg, inv = head(ap_sd, h_wt, h_mt, [b * L for b in range(B + 1)])
    labels = batch["ddg"].to(ddg.dtype).reshape(-1)
    loss = (F.mse_loss(ddg, labels) + F.mse_loss(inv, -labels)) / 2
    return loss, ddg.reshape(B, 1), inv.reshape(B, 1)
