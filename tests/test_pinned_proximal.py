"""The pinned proximal stage of partial repacking: pp_proximal_pinned and everything above it.

Inputs: the committed fixtures g6_prox_L64 and g6_prox_L120 (batch + the sampler's chi0), alone (the B = 1 path of k_prox_init) and as
one pack of 184 rows (two segments of different length).  The pin mask comes from the CPU oracle so that it always bites: with cm the
oracle's clash mask of chi0, every second clash-masked row (by rank) and every third row outside it are fixed -- some rows the
optimiser would move are kept, some stay free.

The reference here is optimize.py:21-73 restated over oracle.ref_cpu.clash_mask / proximal_loss with ``mask & ~fixed`` for ``mask``.
"""
import os

import numpy as np
import pytest
import torch

from .conftest import load_golden, wrapped_absdiff

DEV = "cuda:0"
gpu = pytest.mark.gpu
TAGS = ("L64", "L120")
VTF, TOL, LAMDA = 12.0, 0.5, 1.0
STEPS = 50
REF_STEPS = 10            # L120's marginal hinge flips at step 19 (tests/test_hip_parity.py): 10 steps stay clear of it
SHARD_LENS = (33, 40, 64)


def _g6(tag):
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", f"g6_prox_{tag}.npz"))
    b, g = load_golden(str(z["source_fixture"]))
    return z, b, g[str(z["chi0_key"])].float()


def pin_mask(cm):
    """bool [L] -> bool [L]: every second row of cm (by rank) and every third row outside it."""
    fixed = torch.zeros_like(cm)
    fixed[torch.nonzero(cm).flatten()[1::2]] = True
    fixed[torch.nonzero(~cm).flatten()[::3]] = True
    return fixed


@pytest.fixture(scope="module")
def cases():
    """{tag: (batch, chi0 [1, L, 4], cm [L], fixed [L])} on the host; cm from the CPU oracle."""
    from oracle import ref_cpu as O
    out = {}
    for tag in TAGS:
        _, b, chi0 = _g6(tag)
        cm = O.clash_mask(b, chi0, VTF, TOL)[0, :, 0].clone()
        fixed = pin_mask(cm)
        assert (cm & fixed).any() and (cm & ~fixed).any(), tag
        out[tag] = (b, chi0, cm, fixed)
    return out


def test_the_mask_pins_clashing_rows_of_both_fixtures(cases):
    for tag, (b, chi0, cm, fixed) in cases.items():
        assert chi0.shape == (1, int(b.max_size), 4) and cm.shape == fixed.shape == (int(b.max_size),)
        assert (cm & fixed).any() and (cm & ~fixed).any() and (~cm & fixed).any() and (~cm & ~fixed).any(), tag


@pytest.fixture(scope="module")
def on_gpu(cases):
    """[(batch, chi0, cm, fixed)] on the device, in TAGS order."""
    return [(b.to(DEV), chi0.to(DEV), cm.to(DEV), fixed.to(DEV)) for b, chi0, cm, fixed in cases.values()]


def _pack(items, order=(0, 1)):
    """(packed batch, chi [1, N, 4], cm [N], fixed [N], offsets, padded sizes) of the fixtures in `order`."""
    from packppi_amd.batch import pack
    items = [items[k] for k in order]
    pb = pack([b for b, _, _, _ in items])
    offs = pb["seg_offsets_host"]
    lens = [e - a for a, e in zip(offs[:-1], offs[1:])]
    x = torch.cat([c[:, :n] for (_, c, _, _), n in zip(items, lens)], 1)
    cm = torch.cat([m[:n] for (_, _, m, _), n in zip(items, lens)])
    fixed = torch.cat([f[:n] for (_, _, _, f), n in zip(items, lens)])
    return pb, x, cm, fixed, offs, [int(b.max_size) for b, _, _, _ in items]


# ---- 1. nothing fixed: the bits of the unpinned calls ---------------------------------------------------------------------------
@gpu
def test_all_zero_mask_is_the_unpinned_call(on_gpu):
    from packppi_amd.functional import _ctx_for, proximal_optimizer_packed
    pb, x, _, fixed, offs, _ = _pack(on_gpu)
    assert offs == [0, 64, 184]
    want = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, STEPS, want_traj=True)
    got = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, STEPS, want_traj=True, fixed_mask=torch.zeros_like(fixed),
                                    return_moved=True)
    assert got[0].shape == (STEPS, 1, 184, 4) and got[3].shape == (2, STEPS)
    for t in range(STEPS):
        assert torch.equal(got[0][t], want[0][t]), t
    for k, name in ((1, "last"), (2, "accepted"), (3, "losses")):
        assert torch.equal(got[k], want[k]), name
    assert got[4].any() and not torch.equal(got[1], x)                 # and something was optimised
    for b, chi0, _, f in on_gpu:                                        # B = 1 against Context.proximal
        ctx = _ctx_for(b)
        traj, last, losses = ctx.proximal(chi0, VTF, TOL, LAMDA, STEPS, want_traj=True)
        ptraj, plast, _, plosses = ctx.proximal_packed(chi0, VTF, TOL, LAMDA, STEPS, want_traj=True, fixed=torch.zeros_like(f))
        assert torch.equal(ptraj, traj) and torch.equal(plast, last) and torch.equal(plosses[0], losses)


# ---- 2. the pin -----------------------------------------------------------------------------------------------------------------
@gpu
def test_only_free_rows_of_the_clash_mask_move(on_gpu):
    from packppi_amd.functional import find_clash_mask, proximal_optimizer_packed
    pb, x, cm, fixed, offs, _ = _pack(on_gpu)
    traj, last, acc, losses, moved = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, STEPS, want_traj=True, fixed_mask=fixed,
                                                               return_moved=True)
    assert moved.shape == (1, 184) and moved.dtype == torch.bool
    for s in range(2):
        a, e = offs[s], offs[s + 1]
        assert torch.equal(moved[0, a:e], cm[a:e] & ~fixed[a:e]), s
    still = ~moved[0]
    assert still.any() and moved.any()
    for t in range(STEPS):
        assert torch.equal(traj[t][0, still], x[0, still]), t
    assert torch.equal(last[0, still], x[0, still]) and torch.equal(acc[0, still], x[0, still])
    assert torch.equal(last, traj[-1])
    assert (last[0, moved[0]] != x[0, moved[0]]).any() and (traj[0][0, moved[0]] != x[0, moved[0]]).any()
    assert bool(torch.isfinite(losses).all())
    # B = 1: find_clash_mask reports the same rows
    b, chi0, cm0, f0 = on_gpu[0]
    assert torch.equal(find_clash_mask(b, chi0, VTF, TOL, fixed_mask=f0.reshape(1, -1))[0, :, 0], cm0 & ~f0)
    # everything fixed: nothing moves (no statement about the loss curve: step 0 is recorded by another kernel than the later steps)
    traj, last, acc, _, moved = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, STEPS, want_traj=True,
                                                          fixed_mask=torch.ones_like(fixed), return_moved=True)
    assert not moved.any() and torch.equal(last, x) and torch.equal(acc, x)
    assert all(torch.equal(traj[t], x) for t in range(STEPS))


# ---- 3. packing invariance ------------------------------------------------------------------------------------------------------
@gpu
def test_a_complex_has_the_same_bits_alone_and_in_either_pack(on_gpu):
    from packppi_amd.functional import proximal_optimizer_packed
    solo = [proximal_optimizer_packed(b, chi0, VTF, TOL, LAMDA, STEPS, want_traj=True, fixed_mask=f, return_moved=True)
            for b, chi0, _, f in on_gpu]
    for order in ((0, 1), (1, 0)):
        pb, x, _, fixed, offs, sizes = _pack(on_gpu, order)
        traj, last, acc, losses, moved = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, STEPS, norm_rows=sizes, want_traj=True,
                                                                   fixed_mask=fixed, return_moved=True)
        for s, k in enumerate(order):
            a, e = offs[s], offs[s + 1]
            st, sl, sa, sls, sm = solo[k]
            assert torch.equal(losses[s], sls[0]), (order, s)
            assert torch.equal(traj[:, :, a:e], st[:, :, :e - a]), (order, s)
            assert torch.equal(last[:, a:e], sl[:, :e - a]) and torch.equal(acc[:, a:e], sa[:, :e - a]), (order, s)
            assert torch.equal(moved[:, a:e], sm[:, :e - a]), (order, s)


# ---- 4. against the reference ---------------------------------------------------------------------------------------------------
def pinned_reference(batch, chi0, fixed, num_steps, double=False):
    """optimize.py:21-73 with SC_D_clash_mask & ~fixed: (per-step angles, pre-step losses, mask [1, L, 4])."""
    from oracle import ref_cpu as O
    from packppi_amd.batch import Batch
    if double:
        batch = Batch({k: (v.double() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v) for k, v in batch.items()})
        chi0 = chi0.double()
    with torch.no_grad():
        mask = O.clash_mask(batch, chi0, VTF, TOL) & ~fixed.reshape(1, -1, 1)
    z = chi0 * mask
    x = z.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=1e-2)
    chis, losses = [], []
    for _ in range(num_steps):
        opt.zero_grad()
        loss = O.proximal_loss(batch, x, chi0, mask, z, VTF, TOL, LAMDA)
        loss.backward()
        opt.step()
        chis.append(torch.where(mask, x.detach().clone(), chi0))
        losses.append(loss.item())
    return chis, losses, mask


@gpu
@pytest.mark.parametrize("tag", TAGS)
def test_against_the_restated_reference(tag, cases):
    """The bars test_proximal (tests/test_hip_parity.py) holds these fixtures to: losses rtol 5e-5 against the fp32 reference, angles
    within max(2e-5, 8 x |reference fp32 - reference fp64|) at each step."""
    from packppi_amd.functional import proximal_optimizer
    b, chi0, cm, fixed = cases[tag]
    c32, l32, m32 = pinned_reference(b, chi0, fixed, REF_STEPS)
    c64, l64, m64 = pinned_reference(b, chi0, fixed, REF_STEPS, double=True)
    assert torch.equal(m32, m64) and torch.equal(m32[0, :, 0], cm & ~fixed)
    chis, losses = proximal_optimizer(b.to(DEV), chi0.to(DEV), VTF, TOL, LAMDA, REF_STEPS, fixed_mask=fixed.reshape(1, -1))
    assert len(chis) == REF_STEPS and len(losses) == REF_STEPS
    rel = np.abs(np.array(losses) / np.array(l32) - 1).max()
    div = np.array([float(wrapped_absdiff(a, c).max()) for a, c in zip(c32, c64)])
    d = np.array([float(wrapped_absdiff(g.cpu(), c).max()) for g, c in zip(chis, c32)])
    env = np.maximum(2e-5, 8 * div)
    print(f"pinned proximal {tag}: loss rel {rel:.2e} (vs fp64 reference {np.abs(np.array(losses) / np.array(l64) - 1).max():.2e}); "
          f"angle max {d.max():.2e} rad, reference fp32 vs fp64 max {div.max():.2e} rad; per step "
          + " ".join(f"{v:.1e}" for v in d))
    assert np.allclose(np.array(losses), np.array(l32), rtol=5e-5, atol=1e-7), (tag, rel)
    assert (d <= env).all(), (tag, d.tolist(), env.tolist())
    still = ~m32[0, :, 0]
    assert all(torch.equal(g.cpu()[0, still], chi0[0, still]) for g in chis)


# ---- 5. surface -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = torch.linspace(1, 0, 5)              # 4 sampling steps
    return m


@pytest.fixture(scope="module")
def synth_complexes():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return [protein_to_batch(synth.make_complex(n, 70 + n)).to(DEV) for n in SHARD_LENS]


def synth_mask(i, n):
    """bool [1, n] on the device: rows r with (r + i) % 3 != 0 are kept."""
    return ((torch.arange(n) + i) % 3 != 0).reshape(1, n).to(DEV)


@gpu
def test_repack_is_partial_sampling_then_the_pinned_stage(model, synth_complexes):
    from packppi_amd.batch import pack
    from packppi_amd.functional import proximal_optimizer_packed
    cfg = model.hparams.sample_cfg
    assert cfg.num_steps == STEPS
    prox = (cfg.violation_tolerance_factor, cfg.clash_overlap_tolerance, cfg.lamda, cfg.num_steps)
    cs = []
    for i, c in enumerate(synth_complexes):
        c = type(c)(c)
        c["fixed_mask"], c["complex_key"] = synth_mask(i, SHARD_LENS[i]), 100 + i
        cs.append(c)
    pb = pack(cs)
    mask = pb["fixed_mask"].bool()
    assert mask.shape == (1, 137) and mask.any() and (~mask).any()
    ref = torch.roll(pb.SC_D, 1, dims=1) * pb.SC_D_mask             # angles that are not the batch's own
    for fix_mode in ("hold", "renoise"):
        sample = model.sampling(pb, seed=3, fixed_mask=mask, fixed_chi=ref, fixed_mode=fix_mode)
        want = proximal_optimizer_packed(pb, sample, *prox, fixed_mask=mask)[2]
        got = model.repack(pb, seed=3, fixed_chi=ref, fixed_mode=fix_mode, use_proximal=True)          # batch.fixed_mask is the default
        assert got.shape == (1, 137, 4) and torch.equal(got, want), fix_mode
        assert torch.equal(got[mask], ref[mask]), fix_mode
        assert not torch.equal(got, sample), fix_mode                   # the stage did something
        assert torch.equal(model.repack(pb, mask, seed=3, fixed_chi=ref, fixed_mode=fix_mode), sample), fix_mode
    # B = 1, fixed_chi defaults to SC_D; return_list gives the reference's triple
    c, m0 = synth_complexes[2], synth_mask(2, 64)
    got = model.repack(c, m0, seed=3, use_proximal=True)
    assert torch.equal(got[m0], c.SC_D[m0])
    sample, lst, losses = model.repack(c, m0, seed=3, use_proximal=True, return_list=True)
    assert torch.equal(sample, model.sampling(c, seed=3, fixed_mask=m0))
    assert len(lst) == STEPS and len(losses) == STEPS and all(isinstance(v, float) for v in losses)
    assert all(t.shape == (1, 64, 4) and torch.equal(t[m0], c.SC_D[m0]) for t in lst)
    assert torch.equal(got, lst[-1] if losses[-1] < losses[0] else sample)
    with pytest.raises(ValueError, match="return_list"):
        model.repack(pb, seed=3, use_proximal=True, return_list=True)
    with pytest.raises(ValueError, match="fixed_mask"):
        model.repack(c, seed=3)
    with pytest.raises(ValueError, match="proximal stage has no pin"):
        model.sampling(c, seed=1, fixed_mask=m0, use_proximal=True)


@gpu
def test_c_abi_refusals(on_gpu):
    from packppi_amd import lib as L
    from packppi_amd import synth
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_data
    from packppi_amd.functional import _ctx_for, geometry_plan
    pb, x, _, fixed, _, _ = _pack(on_gpu)
    ctx = _ctx_for(pb)
    ctx.plan.set_clash_params(VTF, TOL)
    lib = L.load()
    fx = fixed.to(torch.uint8).contiguous()
    last, acc, keep = torch.full_like(x, 7.0), torch.full_like(x, 7.0), x.clone()
    losses = torch.full((2, 3), 7.0, device=DEV)
    good = [ctx.handle, x.data_ptr(), fx.data_ptr(), LAMDA, 3, None, None, last.data_ptr(), acc.data_ptr(), losses.data_ptr(), None,
            None]
    for at, bad in ((0, None), (1, None), (2, None), (7, None), (9, None), (4, 0), (4, -2)):
        args = list(good)
        args[at] = bad
        assert lib.pp_proximal_pinned(*args) == 1, (at, bad)
        assert b"pp_proximal_pinned" in lib.pp_last_error()
    padded = collate([protein_to_data(synth.make_complex(n, 40 + n)) for n in (40, 56, 48)]).to(DEV)
    ctx3 = L.Context(geometry_plan(DEV), padded)
    big = [torch.zeros(3, 56, 4, device=DEV) for _ in range(3)]
    assert lib.pp_proximal_pinned(ctx3.handle, big[0].data_ptr(), torch.zeros(168, dtype=torch.uint8, device=DEV).data_ptr(), LAMDA, 3,
                                  None, None, big[1].data_ptr(), big[2].data_ptr(), torch.zeros(3, 3, device=DEV).data_ptr(), None,
                                  None) == 1
    assert b"pp_proximal_pinned" in lib.pp_last_error() and b"padded" in lib.pp_last_error()
    torch.cuda.synchronize()
    # nothing was launched: no output was written
    assert bool((last == 7).all()) and bool((acc == 7).all()) and bool((losses == 7).all()) and torch.equal(x, keep)
    with pytest.raises(ValueError, match="elements"):
        ctx.proximal_packed(x, VTF, TOL, LAMDA, 3, fixed=fx[:-1])
    with pytest.raises(ValueError, match="return_moved"):
        ctx.proximal_packed(x, VTF, TOL, LAMDA, 3, return_moved=True)


# ---- 6. the sharded driver --------------------------------------------------------------------------------------------------------
def test_fixed_masks_need_a_seed():
    """Refused before anything touches a device: there is no model to touch one with."""
    from packppi_amd.parallel import sample_sharded
    with pytest.raises(ValueError, match="fixed_masks needs seed"):
        sample_sharded(None, [], use_proximal=True, fixed_masks={})


@gpu
def test_sharded_repacking_does_not_depend_on_the_layout(model, synth_complexes):
    from packppi_amd.parallel import sample_sharded
    cs = synth_complexes
    masks = {i: synth_mask(i, n) for i, n in enumerate(SHARD_LENS)}
    kw = dict(use_proximal=True, seed=5, lengths=list(SHARD_LENS), fixed_masks=masks)
    one, ids, rows = sample_sharded(model, cs, rank=0, world=1, **kw)
    assert sorted(one) == [0, 1, 2] and ids.tolist() == [0, 1, 2] and rows.shape[0] == 3
    two = {}
    for rank in (0, 1):
        part, _, _ = sample_sharded(model, cs, rank=rank, world=2, **kw)
        assert part and not set(part) & set(two)
        two.update(part)
    loop, _, _ = sample_sharded(model, cs, rank=0, world=1, packed_proximal=False, **kw)          # the per-complex pinned call
    small, _, _ = sample_sharded(model, list(cs), rank=0, world=1, max_rows=70, **kw)             # other groups
    plain, _, _ = sample_sharded(model, cs, rank=0, world=1, seed=5, lengths=list(SHARD_LENS), fixed_masks=masks)
    for i, c in enumerate(cs):
        assert one[i].shape == (1, SHARD_LENS[i], 4)
        assert torch.equal(one[i], two[i]) and torch.equal(one[i], loop[i]) and torch.equal(one[i], small[i]), i
        m = masks[i]
        assert torch.equal(one[i][m], c.SC_D[m]) and torch.equal(plain[i][m], c.SC_D[m]), i
    assert any(not torch.equal(one[i], plain[i]) for i in one)           # the pinned stage moved something
    as_list, _, _ = sample_sharded(model, cs, rank=0, world=1, **dict(kw, fixed_masks=[masks[i] for i in range(3)]))
    assert all(torch.equal(as_list[i], one[i]) for i in one)


# ---- 7. the command lines -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("tool", ["eval_diffusion", "proximal_optimize"])
def test_command_lines_keep_the_residues_outside_the_selection(tool, tmp_path):
    from oracle import ref_cpu as O
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion, proximal_optimize
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    common = ["--input", str(pdb), "--outdir", str(tmp_path / "out"), "--molprobity_clash_loc", "/nonexistent", "--device", "cuda",
              "--repack", "A:5-20"]
    if tool == "eval_diffusion":
        eval_diffusion.main(common + ["--random_weights", "0", "--steps", "4", "--seed", "7", "--use_proximal"])
    else:
        proximal_optimize.main(common)
    read = from_pdb_file(pdb, mse_to_met=True)
    before = protein_to_batch(read)
    after = protein_to_batch(from_pdb_file(tmp_path / "out" / "structure.pdb", mse_to_met=True))
    # what writing UNCHANGED angles costs, from the CPU oracle alone (tests/test_partial_sampling.py::test_surface): its atom14 rebuild
    # of the input's own angles, written and read back like the CLI's structure
    rebuilt = dict(read, atom_positions=O.atom14_coords(before.X, before.residue_type, before.BB_D, before.SC_D)[0].numpy())
    (tmp_path / "rebuilt.pdb").write_text(to_pdb(rebuilt))
    roundtrip = protein_to_batch(from_pdb_file(tmp_path / "rebuilt.pdb", mse_to_met=True))
    kept = torch.ones(60, dtype=torch.bool)
    kept[4:20] = False                                  # chain A is rows 0..29, numbered 1..30
    live = before.SC_D_mask[0].bool()
    sel, rep = live & kept.unsqueeze(-1), live & ~kept.unsqueeze(-1)
    assert sel.any() and rep.any()
    d_in = wrapped_absdiff(after.SC_D[0], before.SC_D[0])
    d_rt = wrapped_absdiff(after.SC_D[0], roundtrip.SC_D[0])
    own = wrapped_absdiff(roundtrip.SC_D[0], before.SC_D[0])[sel].max().item()
    print(f"{tool}: kept residues: max |chi out - oracle round trip| = {d_rt[sel].max().item():.3g} rad, max |chi out - chi in| = "
          f"{d_in[sel].max().item():.3g} (the oracle round trip's own: {own:.3g}); selection: max |chi out - chi in| = "
          f"{d_in[rep].max().item():.3g}")
    # PDB precision, as in test_surface: coordinates rounded to 1e-3 A move an atom by <= 8.7e-4 A; a dihedral's four atoms sit
    # >= 1.2 A from its axis or span bonds >= 1.3 A, so each contributes <= ~1e-3 rad: 5e-3 rad bounds the sum
    assert d_rt[sel].max() < 5e-3                       # the kept angles, written as the oracle writes them
    assert d_in[sel].max() < own + 5e-3                 # ... which is the input's angles, as far as a rebuilt structure holds them
    if tool == "eval_diffusion":
        assert d_in[rep].max() > 0.1                    # the selection was repacked
