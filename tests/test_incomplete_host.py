"""Structures with incomplete side chains, host side: the damage generator (``synth.drop_atoms``), what the fixtures
``g13_incomplete_*`` (the unmodified reference on damaged input, tools/oracle/make_golden_incomplete.py) must contain for the GPU
tests of tests/test_incomplete_gpu.py to bite, the CPU oracle pinned to the reference on such input at the bars of
tests/test_oracle_golden.py, and featurisation against the reference's ``prot_to_data`` on the damaged dicts.

A missing atom has ``atom_mask`` 0 and a NaN position; featurisation turns that into a zero coordinate and ``SC_D_mask`` 0 on every
chi whose four atoms are not all there.  The reference still builds the atoms BEHIND a missing one from chi = 0, so the clash loss
depends on angles whose ``SC_D_mask`` is 0, and its proximal loop -- masked per residue, not per angle -- moves them.
"""
import os

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O
from packppi_amd import constants as rc
from packppi_amd import synth
from packppi_amd.batch import Batch, TENSOR_KEYS, split
from packppi_amd.featurize import protein_to_data
from .conftest import GOLD, load_golden, wrapped_absdiff

CASES = ["L40", "L97", "B2", "1BRS"]
PROT_KEYS = ("atom_positions", "atom_mask", "aaindex", "residue_index", "chain_id", "b_factors")
TIMES = ((1.0, "t1"), (0.5, "t05"), (1.0 / 30, "t30"))
ARG, LYS, GLY = 1, 11, 7


def load_incomplete(tag):
    """(batch, arrays) of one g13 fixture; the arrays also hold ``prot<i>.*`` (the damaged dict) and ``ref<i>.*``."""
    return load_golden("g13_incomplete_" + tag)


def proteins_of(g):
    return [{k: np.asarray(g[f"prot{s}.{k}"]) for k in PROT_KEYS} for s in range(int(g["n_complexes"]))]


def complexes_of(b):
    """The complexes of a fixture batch as B = 1 batches (a padded one keeps its padding rows)."""
    return split(b) if b.residue_type.shape[0] > 1 else [b]


def is_prefix(m):
    """[..., 4] chi mask -> bool: ones first, then zeros."""
    m = m != 0
    return ~(m[..., 1:] & ~m[..., :-1]).any(-1)


# ---- the generator ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_res,seed", [(36, 1436), (40, 1340), (64, 7), (97, 1397)])
def test_drop_atoms_guarantees(n_res, seed):
    p = synth.make_complex(n_res, seed)
    before = {k: np.array(v, copy=True) for k, v in p.items()}
    d = synth.drop_atoms(p, seed + 1)
    for k, v in before.items():                                    # a new dict: the input is untouched
        assert np.array_equal(p[k], v, equal_nan=v.dtype.kind == "f")
    d2 = synth.drop_atoms(p, seed + 1)
    for k in d:                                                    # deterministic in the seed
        assert np.array_equal(d[k], d2[k], equal_nan=np.asarray(d[k]).dtype.kind == "f"), k
    assert not np.array_equal(synth.drop_atoms(p, seed + 2)["atom_mask"], d["atom_mask"])
    aatype, mask, xyz = d["aaindex"], d["atom_mask"], d["atom_positions"]
    table = rc.atom14_mask[aatype]
    assert np.array_equal(aatype, p["aaindex"]) and np.array_equal(d["chain_id"], p["chain_id"])
    assert ((mask == 0) | (table > 0)).all()                       # nothing appears
    assert np.array_equal(np.isnan(xyz).any(-1), mask == 0)        # missing <=> NaN position, as pdb_io writes it
    kept = mask > 0
    assert np.array_equal(xyz[kept], p["atom_positions"][kept])

    kinds = synth.damage_kinds(d)
    assert "other" not in kinds
    n_atoms = table.sum(-1).astype(int)
    for i, k in enumerate(kinds):                                  # the kinds, restated on the mask
        gone = np.flatnonzero((table[i] > 0) & (mask[i] == 0))
        n = n_atoms[i]
        if k == "tail":
            assert 5 <= gone[0] < n and list(gone) == list(range(gone[0], n))
        elif k == "cb_only":
            assert list(gone) == list(range(5, n)) and n > 5
        elif k == "backbone_only":
            assert list(gone) == list(range(4, n)) and aatype[i] != GLY
        elif k == "hole_cb":
            assert list(gone) == [4] and n > 5
        elif k == "hole_inner":
            assert len(gone) == 1 and 5 <= gone[0] < n - 1 and mask[i, gone[0] + 1:n].all()
    for kind in synth.DAMAGE_KINDS:
        assert kinds.count(kind) >= 2, kind
    damaged = np.array([k in synth.DAMAGE_KINDS for k in kinds])
    assert 0.2 * n_res <= damaged.sum() <= 0.36 * n_res             # about a quarter (ten rows is the least that holds every kind twice)
    if np.isin(aatype, (ARG, LYS)).any():
        assert any(k == "hole_cb" and aatype[i] in (ARG, LYS) for i, k in enumerate(kinds))
    chain = d["chain_id"]
    same_next = chain[1:] == chain[:-1]
    assert (damaged[1:] & damaged[:-1] & same_next).any()          # two damaged rows adjacent in sequence
    terminus = np.r_[True, ~same_next] | np.r_[~same_next, True]
    assert (damaged & terminus).any()
    lost = [i for i, k in enumerate(kinds) if k == "masked"]
    assert len(lost) == 1 and not terminus[lost[0]]
    assert damaged[lost[0] - 1] or damaged[lost[0] + 1]
    step = np.diff(d["residue_index"])[same_next]
    assert sorted(step)[-1] == 5 and (step == 1).sum() == len(step) - 1          # one in-chain jump of +4
    at = int(np.flatnonzero(np.diff(d["residue_index"]) == 5)[0])
    bonded = np.linalg.norm(p["atom_positions"][at, 2] - p["atom_positions"][at + 1, 0])
    assert bonded < 1.4                                            # ... across a peptide bond that is still there

    dat = protein_to_data(d)
    assert dat.residue_mask[lost[0]] == 0 and dat.atom_mask[lost[0]].sum() == 0 and int(dat.residue_mask.sum()) == n_res - 1
    assert torch.isfinite(dat.X).all()
    sc, chi_table = dat.SC_D_mask.numpy(), rc.chi_mask_atom14[aatype]
    assert ((sc == 0) | (chi_table > 0)).all()
    for i, k in enumerate(kinds):
        if k in ("cb_only", "backbone_only"):
            assert sc[i].sum() == 0
        if k == "hole_cb" and aatype[i] in (ARG, LYS):
            assert list(sc[i]) == [0, 0, 0, 1]                     # chi4 survives: no prefix of the type's [1, 1, 1, 1]


def test_drop_atoms_refuses_what_it_cannot_damage():
    p = synth.make_complex(9, 3)                                 # ten rows is the least that holds every kind twice
    with pytest.raises(ValueError, match="drop_atoms"):
        synth.drop_atoms(p, 1)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_fixtures_hold_what_the_gpu_tests_need(tag):
    b, g = load_incomplete(tag)
    B, L = b.residue_type.shape
    assert L <= 195 and os.path.getsize(os.path.join(GOLD, f"g13_incomplete_{tag}.npz")) <= 1 << 20
    if tag == "B2":
        assert (B, L) == (2, 40) and b.residue_mask.sum(-1).tolist() == [39.0, 35.0]
    sc = b.SC_D_mask
    live = b.residue_mask.bool()
    assert (live & (sc.sum(-1) > 0) & ~is_prefix(sc)).sum() >= 1
    n_sc = b.atom_mask[..., 4:].sum(-1)
    assert (live & (b.residue_type != GLY) & (n_sc == 0)).sum() >= 2
    grad = g["clash_grad_init"]
    assert ((sc == 0) & (grad != 0)).sum() >= 3
    chi_table = torch.from_numpy(rc.chi_mask_atom14)[b.residue_type]
    assert (grad[chi_table == 0] == 0).all()
    # the GPU test demands an exact zero wherever the reference's gradient is one: every such zero is an angle no active term depends
    # on (zero in the reference's fp64 run too), none a value that fp32 happens to cancel
    g64 = g["clash_grad_init_fp64"]
    assert g64.dtype == torch.float64 and torch.equal(grad == 0, g64 == 0)
    assert (grad.double() - g64).abs().max() < 1e-5 + 1e-4 * g64.abs().max()
    moved = 0
    for s, one in enumerate(complexes_of(b)):
        chi0 = g["init_chi"][s:s + 1]
        c32, c64 = g[f"prox32_chi.{s}"], g[f"prox64_chi.{s}"]
        assert c32.shape == (5, 1, L, 4) and c64.dtype == torch.float64
        assert torch.equal(g[f"prox32_mask.{s}"], g[f"prox64_mask.{s}"])
        moved += int(((c32[-1] != chi0) & (one.SC_D_mask == 0)).sum())
        assert wrapped_absdiff(c32, c64).max() < 1e-6
        l32, l64 = g[f"prox32_losses.{s}"].numpy(), g[f"prox64_losses.{s}"].numpy()
        assert np.abs(l32 / l64 - 1).max() < 1e-6
    assert moved >= 1
    # the initial angles are zero outside SC_D_mask (the reference's noising touches the periodic masks only)
    assert (g["init_chi"][sc == 0] == 0).all()
    for prec in ("32", "64"):
        out = g[f"chi_ode_30_fp{prec}"]
        assert (out[sc == 0] == 0).all()                           # sampling returns exact zeros outside SC_D_mask
    cond = float(wrapped_absdiff(g["chi_ode_30_fp32"], g["chi_ode_30_fp64"])[sc.bool()].max())
    assert cond == pytest.approx(float(g["cond"]), rel=1e-12) and cond < 2e-4
    if tag != "1BRS":                                              # the synthetic ones carry every kind twice
        for p in proteins_of(g):
            kinds = synth.damage_kinds(p)
            assert all(kinds.count(k) >= 2 for k in synth.DAMAGE_KINDS) and kinds.count("masked") == 1
    else:
        natural = np.load(os.path.join(GOLD, "g0_protein_1BRS.npz"))["prot.atom_mask"]
        assert (proteins_of(g)[0]["atom_mask"] <= natural).all()    # the structure's own gaps are kept


@pytest.mark.parametrize("tag", CASES)
def test_featurize_equals_the_reference_on_damaged_dicts(tag):
    b, g = load_incomplete(tag)
    for s, (p, one) in enumerate(zip(proteins_of(g), complexes_of(b))):
        mine = protein_to_data(p)
        n = len(p["aaindex"])
        for k in TENSOR_KEYS:
            ref = g[f"ref{s}.{k}"]
            assert torch.equal(mine[k], ref), (tag, s, k)
            assert torch.equal(one[k][0, :n], ref), (tag, s, k)    # and the stored batch is made of them


# ---- the oracle on incomplete input ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_oracle_graph_and_network(tag, weights):
    b, g = load_incomplete(tag)
    B, L = b.residue_type.shape
    valid = b.residue_mask.bool()
    E_idx, hE = O.encode_static(weights, b)
    assert torch.equal(E_idx[valid], g["E_idx"][valid])
    rows = g["hE0_rows"]
    keep = valid.reshape(-1)[rows]
    assert keep.sum() >= 16
    assert (hE.reshape(B * L, -1, 128)[rows] - g["hE0"])[keep].abs().max() < 2e-5
    chi = g["init_chi"]
    for tval, tn in TIMES:
        t = torch.tensor([tval]).repeat_interleave(B * L)
        score, hV = O.network(weights, b, chi, t)
        assert (hV - g[f"hV_{tn}"])[valid].abs().max() < 5e-5
        assert (score - g[f"score_{tn}"])[valid].abs().max() < 5e-5
    if tag == "L40":
        hV = O.encode_nodes(weights, b, chi, torch.ones(B * L))
        assert (hV - g["hV0_t1"])[valid].abs().max() < 2e-5
        R, tr = O.backbone_frames(b.X)
        mask = b.residue_mask
        ma = mask[..., None] * O._gather_nodes(mask[..., None], E_idx)[..., 0]
        for l in range(3):
            hV, hE = O.ipmp_layer(weights, l, hV, hE, E_idx, R, tr, mask, ma)
            assert (hV - g[f"hV_l{l}_t1"]).abs().max() < 5e-5
            if l < 2:
                assert (hE.reshape(B * L, -1, 128)[rows[:8]] - g[f"hE_l{l}_t1"]).abs().max() < 5e-5


@pytest.mark.parametrize("tag", CASES)
def test_oracle_geometry(tag):
    b, g = load_incomplete(tag)
    chi = g["init_chi"]
    xyz = O.atom14_coords(b.X, b.residue_type, b.BB_D, chi)
    assert (xyz - g["atom14_init"]).abs().max() < 1e-5
    assert torch.equal(xyz[..., :4, :], b.X[..., :4, :])
    pr, grad = O.clash_and_grad(b, chi, 12.0, 0.5)
    assert (pr - g["clash_init"]).abs().max() < 1e-5
    ref = g["clash_grad_init"]
    assert (grad - ref).abs().max() < 1e-5 + 1e-4 * ref.abs().max()
    assert torch.equal(grad == 0, ref == 0)


@pytest.mark.parametrize("tag", CASES)
def test_oracle_sampling_and_proximal(tag, weights):
    b, g = load_incomplete(tag)
    chi = O.sampling(weights, b, g["init_chi"], torch.linspace(1, 0, 31))
    d = wrapped_absdiff(chi, g["chi_ode_30_fp32"])[b.SC_D_mask.bool()]
    assert d.max() < 2e-5, float(d.max())
    assert (chi[b.SC_D_mask == 0] == 0).all()
    for s, one in enumerate(complexes_of(b)):
        chi0 = g["init_chi"][s:s + 1]
        mask = O.clash_mask(one, chi0, 12.0, 0.5)
        assert torch.equal(mask[..., 0], g[f"prox32_mask.{s}"])
        chis, losses = O.proximal_optimizer(one, chi0.clone(), 12.0, 0.5, 1.0, 5)
        assert np.allclose(np.array(losses), g[f"prox32_losses.{s}"].numpy(), rtol=2e-5)
        ref = g[f"prox32_chi.{s}"]
        for n in range(5):
            assert wrapped_absdiff(chis[n], ref[n]).max() < 2e-5
            assert torch.equal(chis[n][~mask], chi0[~mask])
        # the entries outside SC_D_mask that the reference moves, the oracle moves too
        outside = (one.SC_D_mask == 0) & (ref[-1] != chi0)
        assert (chis[-1][outside] != chi0[outside]).all()
