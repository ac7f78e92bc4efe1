"""Partial repacking: pp_sample_partial keeps chosen rows at given angles inside the reverse step.

Shapes as in test_seeded_noise.py: complexes of L = 33 (the smallest K = 32 complex), 40 and 64 under the keys (7, 2^40 + 3, 11),
their pack (N = 137: 16-row tiles straddle complexes), SCHED = linspace(1, 0, 4), and the large pack with more tiles than CUs
(the shallow-ring instance).  Fixed rows: row % 3 != 0 of complex A (tiles with both kinds of row), all of B, none of C.
``fixed_chi`` is SC_D rolled by one residue (and masked), so that nothing passes by copying from the batch.

The pinned values are restated here: the re-noised angle of a fixed entry after step j < n - 1 is add_sc_noise's arithmetic on
fixed_chi with the step-j draws at sigma(schedule[j + 1]); fixed_chi itself after the last step and, in hold mode, at every step.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from .conftest import wrapped_absdiff
from .test_seeded_noise import KEYS, LENS, SCHED, SEED, normals64, words

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_STEPS = len(SCHED) - 1
gpu = pytest.mark.gpu


def fixed_rows(i, n):
    """bool [n]: the fixed rows of complex i (0: row % 3 != 0, 1: all, 2: none)."""
    r = torch.arange(n)
    return (r % 3 != 0) if i == 0 else torch.full((n,), i == 1)


def rolled_chi(c):
    """[1, L, 4]: SC_D of the next residue, masked -- angles that are not the batch's own."""
    return torch.roll(c.SC_D, 1, dims=1) * c.SC_D_mask


@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = SCHED
    return m


@pytest.fixture(scope="module")
def cpu_complexes():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return [protein_to_batch(synth.make_complex(n, 70 + n)) for n in LENS]


@pytest.fixture(scope="module")
def complexes(cpu_complexes):
    cs = [c.to(DEV) for c in cpu_complexes]
    for c, k in zip(cs, KEYS):
        c["complex_key"] = k
        c["complex_keys"] = [k]
    return cs


@pytest.fixture(scope="module")
def large(complexes):
    """(packed batch, keys): 14 complexes of 300 residues and the three small ones, 4337 rows (test_seeded_noise.py's recipe)."""
    from packppi_amd import synth
    from packppi_amd.batch import pack
    from packppi_amd.featurize import protein_to_batch
    two = [protein_to_batch(synth.make_complex(300, 900 + i)).to(DEV) for i in range(2)]
    pb = pack([two[i % 2] for i in range(14)] + list(complexes))
    keys = [100 + i for i in range(14)] + list(KEYS)
    assert pb.max_size == 14 * 300 + 137 > 16 * torch.cuda.get_device_properties(0).multi_processor_count
    return pb, keys


def _ctx(model, batch, keys):
    from packppi_amd.lib import Context
    ctx = Context(model._plan, batch)
    ctx.set_rng_keys(keys)
    return ctx


@pytest.fixture(scope="module")
def pack137(model, complexes):
    """(ctx, batch, fixed [137] bool on the device, fixed_chi [1, 137, 4]) of the pack [A, B, C]."""
    from packppi_amd.batch import pack
    pb = pack(complexes)
    fixed = torch.cat([fixed_rows(i, n) for i, n in enumerate(LENS)]).to(DEV)
    ref = torch.cat([rolled_chi(c) for c in complexes], 1)
    assert ref.shape == (1, 137, 4) and not torch.equal(ref, pb.SC_D)
    return _ctx(model, pb, KEYS), pb, fixed, ref


def initial_state(ctx, batch, fixed, ref, fix_mode):
    """The step-0 state TDiffusionModule.sampling hands to pp_sample_partial."""
    fx = fixed.reshape(1, -1, 1)
    init = ctx.add_noise(torch.where(fx, ref, batch.SC_D), 1.0, SEED)
    return torch.where(fx, ref, init) if fix_mode == "hold" else init


# ---- 1. all rows free: the bits of pp_sample_seeded ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["ode", "sde"])
@pytest.mark.parametrize("case", ["L33", "pack137", "large"])
def test_all_free_is_the_seeded_sampler(case, mode, model, complexes, large, pack137):
    if case == "L33":
        ctx, batch = _ctx(model, complexes[0], [KEYS[0]]), complexes[0]
    elif case == "pack137":
        ctx, batch = pack137[0], pack137[1]
    else:
        ctx, batch = _ctx(model, *large), large[0]
    init = ctx.add_noise(batch.SC_D, 1.0, SEED)
    want = ctx.sample(init, SCHED, mode, seed=SEED)
    assert int(batch.SC_D_mask.sum()) > 0 and torch.isfinite(want).all() and not torch.equal(want, init)
    free = torch.zeros(ctx.n_rows, dtype=torch.uint8, device=DEV)
    for fix_mode in ("hold", "renoise"):
        got, traj = ctx.sample_partial(init, torch.roll(batch.SC_D, 1, dims=1), free, SCHED, mode, SEED, fix_mode, trajectory=True)
        assert traj.shape == (N_STEPS, 1, ctx.n_rows, 4)
        assert torch.equal(got, want) and torch.equal(traj[-1], want)
        assert not torch.equal(traj[0], want)


# ---- 2. the pinned values, bit for bit ----------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,fix_mode", [("ode", "hold"), ("ode", "renoise"), ("sde", "hold"), ("sde", "renoise")])
def test_pinned_values(mode, fix_mode, model, pack137):
    ctx, pb, fixed, ref = pack137
    got, traj = ctx.sample_partial(initial_state(ctx, pb, fixed, ref, fix_mode), ref, fixed, SCHED, mode, SEED, fix_mode,
                                   trajectory=True)
    x = ref.reshape(-1, 4)
    m1, m2 = pb.chi_1pi_periodic_mask.reshape(-1, 4), pb.chi_2pi_periodic_mask.reshape(-1, 4)
    rows = fixed.nonzero().squeeze(1)
    inside = (m1 | m2)[rows]
    assert 0 < rows.numel() < 137 and inside.any() and (~inside).any()
    assert torch.equal(got, traj[-1]) and torch.isfinite(traj).all()
    for j in range(N_STEPS):
        y = traj[j].reshape(-1, 4)[rows]
        if fix_mode == "hold" or j == N_STEPS - 1:
            assert torch.equal(y, x[rows]), j
            continue
        z = ctx.noise(SEED, j)
        sig = model._t_to_sigma(SCHED[j + 1].to(DEV).repeat(137)).unsqueeze(-1)
        want = x + (z[0] * sig) * m1
        want = want + (z[1] * sig) * m2
        want = (want + np.pi) % (2 * np.pi) - np.pi
        d = wrapped_absdiff(y.cpu(), want[rows].cpu())
        print(f"{mode} step {j}: max wrapped |pinned - torch formula| = {d.max().item():.3g}")
        assert d.max() <= 2e-6
        assert torch.equal(y[~inside], x[rows][~inside])               # no noise outside the periodic masks
        assert (y[inside] != x[rows][inside]).all()                    # ... and noise inside them
    # the free rows did move, and they are not the unpinned sampler's
    free = (~fixed).nonzero().squeeze(1)
    live = pb.SC_D_mask.reshape(-1, 4)[free].bool()
    assert live.any() and (traj[0].reshape(-1, 4)[free][live] != traj[-1].reshape(-1, 4)[free][live]).any()


# ---- 3. against the CPU oracle ------------------------------------------------------------------------------------------------
def _restated_noise(i, step):
    """fp32 [2, L_i, 4]: the draws of complex i at `step` from the NumPy generator (nothing read from the device)."""
    return torch.from_numpy(normals64(words(SEED, (LENS[i],), (KEYS[i],), step)).astype(np.float32))


def _restated_noised(x, z, t, m1, m2):
    from oracle import ref_cpu as O
    sig = O.t_to_sigma(torch.as_tensor(t, dtype=torch.float32))
    y = x + (z[0] * sig) * m1
    y = y + (z[1] * sig) * m2
    return torch.where(m1 | m2, O.wrap_pi(y), x)


def _oracle_partial(sd, b, i, fixed, ref, mode, fix_mode):
    """(init [1, L, 4], [n_steps] x [1, L, 4]): the loop of pp_sample_partial composed from the oracle's pieces, the fixed rows
    overwritten after every step with the restated pinned values."""
    from oracle import ref_cpu as O
    L = LENS[i]
    m1, m2 = b["chi_1pi_periodic_mask"].reshape(-1, 4), b["chi_2pi_periodic_mask"].reshape(-1, 4)
    fx, xr = fixed.reshape(-1, 1), ref.reshape(-1, 4)
    init = _restated_noised(torch.where(fx, xr, b["SC_D"].reshape(-1, 4)), _restated_noise(i, -1), 1.0, m1, m2)
    if fix_mode == "hold":
        init = torch.where(fx, xr, init)
    x, traj = init.clone(), []
    static = O.encode_static(sd, b)
    for j in range(N_STEPS):
        time, dt = SCHED[j], SCHED[j] - SCHED[j + 1]
        score, _ = O.network(sd, b, x.reshape(1, L, 4), time.repeat_interleave(L), static)
        score = score.reshape(-1, 4)
        z = _restated_noise(i, j)
        x = O.reverse_step(x, score, time, dt, m1, mode, z[0])
        x = O.reverse_step(x, score, time, dt, m2, mode, z[1])
        x = O.wrap_pi(x) * b["SC_D_mask"].reshape(-1, 4)
        pinned = _restated_noised(xr, z, SCHED[j + 1], m1, m2) if fix_mode == "renoise" and j < N_STEPS - 1 else xr
        x = torch.where(fx, pinned, x)
        traj.append(x.reshape(1, L, 4).clone())
    return init.reshape(1, L, 4), traj


@gpu
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_against_the_cpu_oracle(mode, model, weights, cpu_complexes, pack137):
    """Free entries with SC_D_mask, every step of chi_traj: within 1e-4 rad (the project's figure for pp_sample against the oracle)
    of the composed oracle loop.  Controls: hold, renoise and the unpinned sampler differ by more than 1e-3 rad somewhere."""
    from packppi_amd.batch import unpack
    ctx, pb, fixed, ref = pack137
    results = {}
    for fix_mode in ("hold", "renoise"):
        oracle = [_oracle_partial(weights, b, i, fixed_rows(i, n), rolled_chi(b), mode, fix_mode)
                  for i, (b, n) in enumerate(zip(cpu_complexes, LENS))]
        init = torch.cat([o[0] for o in oracle], 1).to(DEV)
        got, traj = ctx.sample_partial(init, ref, fixed, SCHED, mode, SEED, fix_mode, trajectory=True)
        results[fix_mode] = got
        worst, n_free = 0.0, 0
        for j in range(N_STEPS):
            for i, part in enumerate(unpack(pb, traj[j])):
                sel = (~fixed_rows(i, LENS[i])).reshape(1, -1, 1) & cpu_complexes[i].SC_D_mask.bool()
                if sel.any():
                    worst = max(worst, wrapped_absdiff(part.cpu(), oracle[i][1][j])[sel].max().item())
                    n_free += int(sel.sum())
        print(f"{mode} {fix_mode}: max wrapped |device - oracle| over {n_free} free entries x steps = {worst:.3g}")
        assert n_free > 0 and worst < 1e-4
    results["none"] = ctx.sample(ctx.add_noise(pb.SC_D, 1.0, SEED), SCHED, mode, seed=SEED)
    sel = (~fixed).reshape(1, -1, 1) & pb.SC_D_mask.bool()
    assert sel.any()
    for a, b in (("hold", "renoise"), ("hold", "none"), ("renoise", "none")):
        d = wrapped_absdiff(results[a].cpu(), results[b].cpu())[sel.cpu()].max().item()
        print(f"{mode}: max wrapped |{a} - {b}| on free entries = {d:.3g}")
        assert d > 1e-3, (a, b)


# ---- 4. packing invariance ----------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode,fix_mode", [("ode", "hold"), ("ode", "renoise"), ("sde", "renoise")])
def test_packing_invariance(mode, fix_mode, model, complexes):
    """sampling(seed=5, fixed_mask=...) gives every complex the same bits alone, in the pack [A, B, C] (mask handed over) and in the
    pack [C, A, B] (mask carried by pack() as the complexes' fixed_mask key)."""
    from packppi_amd.batch import pack, unpack
    masks = [fixed_rows(i, n).reshape(1, n).to(DEV) for i, n in enumerate(LENS)]
    refs = [rolled_chi(c) for c in complexes]
    model.hparams.sample_cfg.mode = mode
    try:
        alone = [model.sampling(c, seed=5, fixed_mask=m, fixed_chi=r, fixed_mode=fix_mode) for c, m, r in zip(complexes, masks, refs)]
        pb = pack(complexes)
        abc = unpack(pb, model.sampling(pb, seed=5, fixed_mask=torch.cat(masks, 1), fixed_chi=torch.cat(refs, 1), fixed_mode=fix_mode))
        order = (2, 0, 1)
        tagged = []
        for i in order:
            c = type(complexes[i])(complexes[i])
            c["fixed_mask"] = masks[i]
            tagged.append(c)
        pc = pack(tagged)
        assert torch.equal(pc.fixed_mask, torch.cat([masks[i] for i in order], 1))
        cab = dict(zip(order, unpack(pc, model.sampling(pc, seed=5, fixed_chi=torch.cat([refs[i] for i in order], 1), fixed_mode=fix_mode))))
        for i in range(3):
            assert alone[i].shape == (1, LENS[i], 4) and torch.isfinite(alone[i]).all()
            assert torch.equal(alone[i], abc[i]) and torch.equal(alone[i], cab[i])
        assert not torch.equal(alone[0], model.sampling(complexes[0], seed=6, fixed_mask=masks[0], fixed_chi=refs[0], fixed_mode=fix_mode))
    finally:
        model.hparams.sample_cfg.mode = "ode"


# ---- the exact-fp32 library (its own node-update kernel) -----------------------------------------------------------------------
@gpu
def test_exact_fp32_library():
    """All-free equality, the pinned values and the oracle comparison once more on libpackppi_hip.f32.so, in a fresh child."""
    from packppi_amd.build import other_variant_path
    lib = other_variant_path()
    if os.environ.get("PACKPPI_LIB"):
        pytest.skip("already a child run")
    if not os.path.exists(lib):
        pytest.skip(f"{os.path.basename(lib)} not built (__graft_entry__.build() builds it)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_all_free_is_the_seeded_sampler or test_pinned_values or test_against_the_cpu_oracle"],
                       env=dict(os.environ, PACKPPI_LIB=lib), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert "12 passed" in r.stdout


# ---- 5. surface ---------------------------------------------------------------------------------------------------------------
@gpu
def test_surface(model, complexes, pack137, tmp_path):
    from packppi_amd import lib as L
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    c, mask, ref = complexes[0], fixed_rows(0, LENS[0]).reshape(1, -1).to(DEV), rolled_chi(complexes[0])
    with pytest.raises(ValueError, match="needs seed"):
        model.sampling(c, fixed_mask=mask)
    with pytest.raises(ValueError, match="exclude each other"):
        model.sampling(c, seed=1, fixed_mask=mask, sde_noise=torch.zeros(3, 2, 33, 4, device=DEV))
    with pytest.raises(ValueError, match="proximal stage has no pin"):
        model.sampling(c, seed=1, fixed_mask=mask, use_proximal=True)
    with pytest.raises(ValueError, match="fixed_mode"):
        model.sampling(c, seed=1, fixed_mask=mask, fixed_mode="freeze")
    # the C ABI: null arguments, chi_ref == chi, unknown fix_mode / mode -> PP_ERR_INVALID (1), nothing launched
    ctx, pb, fixed, pref = pack137
    lib = L.load()
    chi = ctx.add_noise(pb.SC_D, 1.0, SEED)
    fx = fixed.to(torch.uint8).contiguous()
    sched = np.ascontiguousarray(SCHED.numpy(), dtype=np.float32)
    good = [ctx.handle, chi.data_ptr(), pref.contiguous().data_ptr(), fx.data_ptr(), 1, sched.ctypes.data, len(sched), 0, SEED, None, None]
    for at, bad in ((0, None), (1, None), (2, None), (3, None), (5, None), (2, chi.data_ptr()), (4, 2), (4, -1), (7, 2)):
        args = list(good)
        args[at] = bad
        assert lib.pp_sample_partial(*args) == 1, (at, bad)
        assert b"pp_sample_partial" in lib.pp_last_error()
    torch.cuda.synchronize()
    # sampling: the fixed rows are fixed_chi bit for bit, the free rows are not; the trajectory has one slice per step
    for fix_mode in ("hold", "renoise"):
        out, traj = model.sampling(c, seed=3, fixed_mask=mask, fixed_chi=ref, fixed_mode=fix_mode, return_trajectory=True)
        assert out.shape == (1, 33, 4) and traj.shape == (N_STEPS, 1, 33, 4) and torch.equal(traj[-1], out)
        assert mask.any() and torch.equal(out[mask], ref[mask])
        live = c.SC_D_mask.bool() & ~mask.unsqueeze(-1)
        assert live.any() and (out[live] != ref[live]).any()
    assert torch.equal(model.sampling(c, seed=3, fixed_mask=mask)[mask], c.SC_D[mask])          # fixed_chi defaults to batch.SC_D
    # the command line: residues outside --repack keep the input's angles
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    eval_diffusion.main(["--input", str(pdb), "--outdir", str(tmp_path / "out"), "--molprobity_clash_loc", "/nonexistent",
                         "--device", "cuda", "--random_weights", "0", "--steps", "4", "--seed", "7", "--repack", "A:5-20"])
    read = from_pdb_file(pdb, mse_to_met=True)
    before = protein_to_batch(read)
    after = protein_to_batch(from_pdb_file(tmp_path / "out" / "structure.pdb", mse_to_met=True))
    # what writing UNCHANGED angles costs, from the CPU oracle alone: its atom14 rebuild of the input's own angles (ideal rigid groups
    # on the backbone frames: atoms move by up to 0.05 A against the file), written and read back like the CLI's structure
    from oracle import ref_cpu as O
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
    # PDB precision: coordinates rounded to 1e-3 A move an atom by <= 8.7e-4 A; a dihedral's four atoms sit >= 1.2 A from its axis
    # or span bonds >= 1.3 A, so each contributes <= ~1e-3 rad: 5e-3 rad bounds the sum
    print(f"kept residues: max |chi out - oracle round trip| = {d_rt[sel].max().item():.3g} rad, max |chi out - chi in| = "
          f"{d_in[sel].max().item():.3g} (the oracle round trip's own: {own:.3g}); repacked: max |chi out - chi in| = {d_in[rep].max().item():.3g}")
    assert d_rt[sel].max() < 5e-3                       # the kept angles, written as the oracle writes them
    assert d_in[sel].max() < own + 5e-3                 # ... which is the input's angles, as far as a rebuilt structure holds them
    assert d_in[rep].max() > 0.1                        # the selection was repacked
    with pytest.raises(SystemExit):
        eval_diffusion.main(["--input", str(pdb), "--outdir", str(tmp_path / "x"), "--molprobity_clash_loc", "/nonexistent",
                             "--random_weights", "0", "--repack", "A:5-20"])         # --repack needs --seed
