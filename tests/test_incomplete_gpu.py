"""GPU: every kernel that reads ``atom_mask`` or ``SC_D_mask`` on structures with incomplete side chains.

Reference: the unmodified reference's tensors on ``synth.drop_atoms`` inputs (fixtures g13_incomplete_*, pinned and described by
tests/test_incomplete_host.py), at the bars the complete-structure tests of tests/test_hip_parity.py hold the same kernels to.  The
inputs carry what no complete structure has: chi masks that are proper prefixes of the type's table and ones that are no prefix at all,
non-GLY rows without a side-chain atom (n_sc = 0), holes with atoms behind them -- the clash gradient is then NON-zero on angles
whose ``SC_D_mask`` is 0, and the reference's proximal loop moves them --, a row masked mid-chain next to damaged rows, a numbering gap
inside a chain.  The kernels without a reference run against the restatements of their own test modules on a damaged complex.

PACKPPI_INCOMPLETE_REPORT=<file> appends the measured distances (profiles/r24_incomplete_inputs.txt).
"""
import os

import numpy as np
import pytest
import torch

from .conftest import wrapped_absdiff
from .test_incomplete_host import CASES, TIMES, complexes_of, is_prefix, load_incomplete

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x1234_5678_9abc_def0
VTF, TOL, LAMDA = 12.0, 0.5, 1.0


def _report(line):
    print(line)
    path = os.environ.get("PACKPPI_INCOMPLETE_REPORT")
    if path:
        libname = os.path.basename(os.environ.get("PACKPPI_LIB") or "libpackppi_hip.so")
        with open(path, "a") as fh:
            fh.write(f"{libname:24s} {line}\n")


@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    return TDiffusionModule(weights, device=DEV)


def _damaged(n_res, seed, damage_seed):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.drop_atoms(synth.make_complex(n_res, seed), damage_seed))


def _complete(n_res, seed):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.make_complex(n_res, seed))


# ---- against the reference's tensors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_graph_and_edge_embedding(tag, model):
    b, g = load_incomplete(tag)
    B, L = b.residue_type.shape
    E, hE = model._context(b.to(DEV)).graph()
    E, hE = E.cpu(), hE.cpu()
    valid = b.residue_mask.bool()
    assert torch.equal(E[valid], g["E_idx"][valid])
    rows = g["hE0_rows"]
    real = (torch.gather(b.residue_mask[:, None].expand(-1, L, -1), 2, E) > 0) & valid[..., None]
    real = real.reshape(B * L, -1)[rows]
    assert real.any(-1).sum() >= 16
    d = (hE.reshape(B * L, -1, 128)[rows] - g["hE0"])[real].abs().max()
    _report(f"{tag:5s} hE0 {float(d):.2e}")
    assert d < 2e-5


@pytest.mark.parametrize("tag", CASES)
def test_network_at_three_times(tag, model):
    b, g = load_incomplete(tag)
    gb = b.to(DEV)
    B, L = b.residue_type.shape
    valid = b.residue_mask.bool()
    chi = g["init_chi"].to(DEV)
    for tval, tn in TIMES:
        t = torch.tensor([tval]).repeat_interleave(B * L)
        score, hV = model.network(gb, chi, t)
        dh = (hV.cpu() - g[f"hV_{tn}"])[valid].abs().max()
        ds = (score.cpu() - g[f"score_{tn}"])[valid].abs().max()
        _report(f"{tag:5s} {tn:3s} hV {float(dh):.2e} score {float(ds):.2e}")
        assert dh < 1e-4, tn
        assert ds < 5e-5, tn


@pytest.mark.parametrize("tag", CASES)
def test_atom14_clash_and_gradient(tag):
    from packppi_amd.functional import _ctx_for, compute_residue_clash, get_atom14_coords
    b, g = load_incomplete(tag)
    gb = b.to(DEV)
    chi = g["init_chi"].to(DEV)
    xyz = get_atom14_coords(gb.X, gb.residue_type, gb.BB_D, chi).cpu()
    assert (xyz - g["atom14_init"]).abs().max() < 2e-5
    assert torch.equal(xyz[..., :4, :], b.X[..., :4, :])
    pr = compute_residue_clash(gb, chi, VTF, TOL).cpu()
    assert (pr - g["clash_init"]).abs().max() < 2e-5
    # a non-GLY row without a side-chain atom scores 0 / 1e-10 = 0, not NaN
    bare = b.residue_mask.bool() & (b.atom_mask[..., 4:].sum(-1) == 0)
    assert bare.sum() >= 2 and (pr[bare] == 0).all() and torch.isfinite(pr).all()
    _, grad = _ctx_for(gb).clash(chi, VTF, TOL, need_grad=True)
    grad, ref = grad.cpu(), g["clash_grad_init"]
    d = (grad - ref).abs().max()
    outside = (b.SC_D_mask == 0) & (ref != 0)
    _report(f"{tag:5s} gradient {float(d):.2e} (max |ref| {float(ref.abs().max()):.2e}; {int(outside.sum())} entries outside SC_D_mask)")
    assert d < 1e-5 + 1e-4 * ref.abs().max()
    assert (grad[ref == 0] == 0).all()
    assert outside.sum() >= 3 and (grad[outside] != 0).all()


@pytest.mark.parametrize("tag", CASES)
def test_ode_30_steps(tag, model):
    b, g = load_incomplete(tag)
    ctx = model._context(b.to(DEV))
    out = ctx.sample(g["init_chi"].to(DEV), torch.linspace(1, 0, 31)).cpu()
    mask = b.SC_D_mask.bool()
    cond = float(g["cond"])
    d64 = float(wrapped_absdiff(out, g["chi_ode_30_fp64"])[mask].max())
    d32 = float(wrapped_absdiff(out, g["chi_ode_30_fp32"])[mask].max())
    _report(f"{tag:5s} ode30 |this - ref64| {d64:.2e} |this - ref32| {d32:.2e} cond {cond:.2e}")
    assert d64 < max(1e-4, 3 * cond), (d64, cond)
    assert d32 < max(1e-4, 3 * cond), (d32, cond)
    assert (out[~mask] == 0).all()
    assert (mask & ~is_prefix(b.SC_D_mask)[..., None]).any()           # ... also on rows whose mask is no prefix
    assert ctx.saturated() == 0


@pytest.mark.parametrize("tag", CASES)
def test_five_proximal_steps(tag):
    from packppi_amd.functional import _ctx_for
    b, g = load_incomplete(tag)
    for s, one in enumerate(complexes_of(b)):
        chi0 = g["init_chi"][s:s + 1]
        ref, ref_losses = g[f"prox32_chi.{s}"], g[f"prox32_losses.{s}"].numpy()
        mask = g[f"prox32_mask.{s}"].bool()[..., None].expand(-1, -1, 4)
        traj, last, losses = _ctx_for(one.to(DEV)).proximal(chi0.to(DEV), VTF, TOL, LAMDA, 5)
        traj, last, losses = traj.cpu(), last.cpu(), losses.cpu().numpy()
        _report(f"{tag:5s} proximal[{s}] loss rel {np.abs(losses / ref_losses - 1).max():.2e} "
                f"angle {float(wrapped_absdiff(traj, ref).max()):.2e} rad")
        assert np.allclose(losses, ref_losses, rtol=2e-5, atol=1e-7), (losses, ref_losses)
        for n in range(5):
            assert wrapped_absdiff(traj[n], ref[n]).max() < 2e-5, n
            assert torch.equal(traj[n][~mask], chi0[~mask]), n
        assert torch.equal(last, traj[-1])
        # the reference's mask is per residue: entries outside SC_D_mask that it moves must move here too
        moved = (one.SC_D_mask == 0) & (ref[-1] != chi0)
        assert (last[moved] != chi0[moved]).all()
    assert sum(int(((g[f"prox32_chi.{s}"][-1] != g["init_chi"][s:s + 1]) & (one.SC_D_mask == 0)).sum())
               for s, one in enumerate(complexes_of(b))) >= 1


# ---- packing: a damaged complex between two complete ones -------------------------------------------------------------------------
@pytest.fixture(scope="module")
def trio():
    """(complete 40, damaged 64, complete 33) on the device, each with its key."""
    cs = [_complete(40, 77).to(DEV), _damaged(64, 11, 64).to(DEV), _complete(33, 78).to(DEV)]
    for c, k in zip(cs, (3, 2 ** 40 + 5, 9)):
        c["complex_key"] = k
        c["complex_keys"] = [k]
    return cs


@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_packed_sampling_gives_the_damaged_complex_its_bits(mode, model, trio):
    from packppi_amd.batch import pack, unpack
    model.hparams.sample_cfg.mode = mode
    model.schedule = torch.linspace(1, 0, 5)
    try:
        alone = model.sampling(trio[1], seed=5)
        pb = pack(trio)
        assert pb.seg_offsets_host == [0, 40, 104, 137]
        mid = unpack(pb, model.sampling(pb, seed=5))[1]
    finally:
        model.hparams.sample_cfg.mode = "ode"
    assert torch.isfinite(alone).all() and torch.equal(alone, mid)
    m = trio[1].SC_D_mask.bool()
    assert (alone[~m] == 0).all() and (alone[m] != 0).any()


def test_packed_proximal_gives_the_damaged_complex_its_bits(trio):
    from .test_packed_proximal import _check_pack
    g = torch.Generator().manual_seed(5)
    chis = [((torch.rand(1, int(b.max_size), 4, generator=g) * 2 - 1) * 3.0).to(DEV) * b.SC_D_mask for b in trio]
    losses = _check_pack(trio, chis, steps=5)
    assert all(torch.isfinite(ls).all() for ls in losses)
    # the damaged complex moves entries outside SC_D_mask in the pack as it does alone (checked bit for bit above): they do move
    from packppi_amd.functional import _ctx_for
    _, last, _ = _ctx_for(trio[1]).proximal(chis[1], VTF, TOL, LAMDA, 5)
    assert ((last != chis[1]) & (trio[1].SC_D_mask == 0)).any()


# ---- live rows, seeded noising ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CASES)
def test_live_rows(tag, model):
    from packppi_amd import synth
    from .test_incomplete_host import proteins_of
    b, g = load_incomplete(tag)
    ctx = model._context(b.to(DEV))
    got = ctx.live_rows().cpu().numpy()
    rm, sc = b.residue_mask.reshape(-1).numpy(), b.SC_D_mask.reshape(-1, 4).numpy()
    want = np.flatnonzero((rm != 0) & (sc != 0).any(-1)).astype(np.int32)
    assert got.dtype == np.int32 and np.array_equal(got, want)
    L = b.residue_type.shape[1]
    dead = [s * L + i for s, p in enumerate(proteins_of(g)) for i, k in enumerate(synth.damage_kinds(p))
            if k in ("backbone_only", "cb_only", "masked")]
    assert len(dead) >= 5 and not np.isin(dead, got).any()
    nonprefix = np.flatnonzero(~is_prefix(b.SC_D_mask).reshape(-1).numpy())
    assert len(nonprefix) >= 1 and np.isin(nonprefix, got).all()


def _noised_f32(x, z, sigma, m1, m2):
    """pp_noised_angle restated in float32, every operation rounded on its own: x += (z1 sigma) m1, x += (z2 sigma) m2, wrap."""
    f = np.float32
    x = (x + (z[0] * f(sigma)) * m1.astype(f)).astype(f)
    x = (x + (z[1] * f(sigma)) * m2.astype(f)).astype(f)
    PI, TWO_PI = f(3.14159274101257324), f(6.28318548202514648)
    r = np.fmod((x + PI).astype(f), TWO_PI)
    r = np.where(r < 0, (r + TWO_PI).astype(f), r)
    return (r - PI).astype(f)


@pytest.mark.parametrize("tag", CASES)
def test_seeded_noising(tag, model):
    """pp_add_noise_seeded: the draws are the generator restated in tests/test_seeded_noise.py word for word; the noised angles are
    the torch formula of test_seeded_noise.test_initial_noising on those draws (its bar, 2e-6 wrapped) and the float32 restatement of
    the kernel's own statement; an entry outside both periodic masks -- every entry outside SC_D_mask -- comes back untouched."""
    from packppi_amd.lib import Context
    from .test_seeded_noise import normals64, words
    b, g = load_incomplete(tag)
    B, L = b.residue_type.shape
    gb = b.to(DEV)
    ctx = Context(model._plan, gb)
    keys = [11 + s for s in range(B)]
    ctx.set_rng_keys(keys)
    z, w = ctx.noise(SEED, -1, want_words=True)
    assert np.array_equal(w.cpu().numpy().view(np.uint32), words(SEED, [L] * B, keys, -1))
    assert np.abs(z.cpu().numpy().astype(np.float64) - normals64(w.cpu().numpy().view(np.uint32))).max() <= 1e-5
    # angles outside the masks that are not zero, so that "untouched" is not "zeroed"
    x = b.SC_D.clone()
    x[b.SC_D_mask == 0] = 0.25
    got = ctx.add_noise(x.to(DEV), 1.0, SEED).cpu().reshape(-1, 4)
    x = x.reshape(-1, 4)
    m1, m2 = b.chi_1pi_periodic_mask.reshape(-1, 4), b.chi_2pi_periodic_mask.reshape(-1, 4)
    assert torch.equal((m1 | m2), b.SC_D_mask.reshape(-1, 4) != 0)
    outside = ~(m1 | m2)
    assert outside.sum() > 4 * (~b.residue_mask.bool()).sum() and torch.equal(got[outside], x[outside])
    assert (got[~outside] != x[~outside]).all()
    sig = model._t_to_sigma(torch.ones(x.shape[0]))[:, None]
    zc = z.cpu()
    want = x + (zc[0] * sig) * m1
    want = want + (zc[1] * sig) * m2
    want = (want + np.pi) % (2 * np.pi) - np.pi
    d = wrapped_absdiff(got, want)[~outside].max()
    lo, hi = np.log(0.01 * np.pi), np.log(np.pi)                       # sigma(t = 1) as pp_add_noise_seeded forms it, in float32
    sigma = np.exp(np.float32(lo) + np.float32(hi - lo) * np.float32(1.0), dtype=np.float32)
    restated = _noised_f32(x.numpy(), zc.numpy(), sigma, m1.numpy(), m2.numpy())
    differ = int((restated[~outside.numpy()] != got.numpy()[~outside.numpy()]).sum())
    print(f"{tag}: max wrapped |add_noise - torch formula| = {float(d):.3g}; entries that differ from the float32 restatement {differ}")
    assert d <= 2e-6
    assert differ == 0


# ---- the kernels without a reference, against the restatements of their own modules ----------------------------------------------------
def test_shell_on_a_damaged_complex_alone_and_packed():
    """pp_ctx_shell, both modes (atom mode reads atom_mask and the zeroed coordinates of missing atoms), on the damaged complex and on
    the pack (complete, damaged, complete) with the seeds in the damaged segment: the matrix of tests/test_shell_gpu.py."""
    from packppi_amd.batch import pack
    from .test_shell_gpu import _run_matrix, _seed_sets
    d = _damaged(64, 11, 64).to(DEV)
    am = d.atom_mask[0].cpu().numpy()
    bare = np.flatnonzero((am[:, :4].sum(-1) == 4) & (am[:, 4:].sum(-1) == 0) & (d.residue_type[0].cpu().numpy() != 7))
    gone = np.flatnonzero(am.sum(-1) == 0)
    assert len(bare) >= 2 and len(gone) == 1
    sets = _seed_sets(0, 64, 64)
    for name, rows in (("a backbone-only row", bare[:1]), ("the masked row", gone)):
        sets[name] = np.zeros(64, np.uint8)
        sets[name][rows] = 1
    assert _run_matrix(d, [0, 64], sets) == 2 * 2 * 3 * 6 * 2
    pb = pack([_complete(97, 267).to(DEV), d, _complete(97, 267).to(DEV)])
    offs = pb.seg_offsets_host
    assert offs == [0, 97, 161, 258]
    sets = _seed_sets(97, 161, 258)
    sets["every row"] = np.ones(258, np.uint8)
    _run_matrix(pb, offs, sets)


def test_recombination_local_energies_on_a_damaged_complex():
    """pp_ensemble_recombine on four uniform decoys of the damaged complex against the fp64 restatement of tests/test_recombine_host.py:
    the local energies (rows with n_sc = 0 weigh 1 / 1e-10 x 0, partner lists from the extents of the atoms that are there), the
    descent and the local optimum, at that module's bounds."""
    from . import test_recombine_gpu as R
    from . import test_recombine_host as H

    class DamagedCase(H.Case):
        def __init__(self):
            self.name, self.n, self.D = "damaged64", 64, 4
            self.b = _damaged(64, 11, 64)
            self.chis = H.decoy_angles(self.b, 64, 4, "uniform")

    d = R.Dev(DamagedCase())
    R.check_arithmetic(d)
    R.check_is_a_recombination(d)
    R.check_descent(d)
    R.check_local_optimum(d)
    still = (d.gb.SC_D_mask[0] == 0).all(-1)
    assert int(still.sum()) >= 10 and bool((d.rec.pick[still] == d.start).all())


def test_ensemble_reduce_on_a_damaged_complex(model):
    """pp_ensemble_reduce over five seeded decoys of the damaged complex against the fp64 restatement of tests/test_ensemble_gpu.py, at
    its bounds.  The angles outside SC_D_mask are NOT zero here (the proximal stage leaves them so): they must not enter the consensus
    or the deviation."""
    from packppi_amd.batch import replicate
    from packppi_amd.lib import Context
    from .test_ensemble_gpu import MEAN_TOL, _host, _wrapped, consensus64, scores64
    D, n = 5, 64
    c = _damaged(64, 11, 64).to(DEV)
    pb = replicate(c, D, key=2 ** 40 + 5)
    model.schedule = torch.linspace(1, 0, 4)
    chi = model.sampling(pb, seed=SEED)
    g = torch.Generator().manual_seed(3)
    junk = ((torch.rand(1, D * n, 4, generator=g) * 2 - 1) * 3.0).to(DEV)
    chi = torch.where(pb.SC_D_mask != 0, chi, junk)
    ctx = Context(model._plan, pb)
    per_res = ctx.clash(chi)
    r = ctx.ensemble_reduce(chi, D, per_res=per_res, select="clash")
    mask, m1pi, offs = _host(pb)
    x = chi[0].cpu().numpy()
    valid = (mask != 0)[:n]
    assert valid.sum() > 60 and (~valid).sum() > 100
    mean_ref, res_ref = consensus64(x, mask, m1pi, offs, D)
    mean, res = r.mean[0].cpu().numpy(), r.resultant[0].cpu().numpy()
    cmp = valid & (res_ref >= 1e-6)
    assert (valid & ~cmp).sum() == 0
    P = np.where(m1pi[:n], np.pi, 2.0 * np.pi)
    dm = _wrapped(mean.astype(np.float64) - mean_ref, P)[cmp].max()
    dr = np.abs(res.astype(np.float64) - res_ref)[valid].max()
    print(f"damaged64: max |mean - ref| {dm:.3e} rad, max |resultant - ref| {dr:.3e}")
    assert dm <= MEAN_TOL and dr <= 1e-6
    assert (mean[~valid] == 0).all() and (res[~valid] == 0).all()
    dev_ref, clash_ref = scores64(x, mean, mask, m1pi, per_res.reshape(-1).cpu().numpy(), offs, D)
    dev, clash = r.dev.cpu().numpy(), r.clash.cpu().numpy()
    assert np.all(np.abs(dev - dev_ref) <= 1e-9 * np.abs(dev_ref) + 1e-12)
    assert np.all(np.abs(clash - clash_ref) <= 1e-9 * np.abs(clash_ref) + 1e-12)
    best = int(r.best[0])
    assert best == int(np.argmin(clash)) and torch.equal(r.chi_best[0], chi[0, best * n:(best + 1) * n])


@pytest.fixture(scope="module")
def keyed(model, trio):
    """(context, batch, lengths) of the damaged complex alone and of the pack (complete, damaged, complete), with the keys set."""
    from packppi_amd.batch import pack
    from .test_guided_gpu import _ctx
    pb = pack(trio)
    return ((_ctx(model, trio[1], trio[1]["complex_keys"]), trio[1], (64,)),
            (_ctx(model, pb, pb["complex_keys"]), pb, (40, 64, 33)))


def test_one_guided_nudge_on_a_damaged_complex(keyed, trio):
    """One nudge of pp_sample_guided in isolation against the restatement of tests/test_guided_host.py (2e-6 wrapped, its bar): the clash
    gradient is non-zero on entries outside SC_D_mask, which are not movable and must come back bit for bit."""
    from .test_guided_gpu import one_nudge
    from .test_guided_host import CAP, nudge
    cpu = [type(c)({k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in c.items()}) for c in trio]
    results = []
    for (ctx, b, lens), cs in zip(keyed, ([cpu[1]], cpu)):
        front, chi = one_nudge(ctx, b, 0.05, CAP)
        for c, x, y in zip(cs, torch.split(front.cpu(), list(lens), 1), torch.split(chi.cpu(), list(lens), 1)):
            want, _, mov, G = nudge(c, x, 0.05, CAP)
            assert mov.any() and torch.equal(y[~mov], x[~mov])
            d = float(wrapped_absdiff(y, want).max())
            print(f"L = {x.shape[1]}: max wrapped |device - restated nudge| = {d:.3g} over {int(mov.sum())} movable lanes")
            assert d <= 2e-6
            if x.shape[1] == 64:
                held = (c.SC_D_mask == 0) & (G != 0)
                assert held.sum() >= 3 and not (held & mov).any()
                results.append(y)
    assert torch.equal(results[0], results[1])                    # alone and in the pack: the same bits


def test_one_corrector_on_a_damaged_complex(keyed, trio):
    """One corrector of pp_sample_corrected in isolation, at the bounds of tests/test_corrector_gpu.py: both norms are sums over the
    movable entries only -- the device's score is not zero outside SC_D_mask --, the update is the restated one, everything else
    comes back bit for bit."""
    from oracle import ref_cpu as O
    from .test_corrector_gpu import one_corrector
    from .test_corrector_host import SNR, corrector_noise64, step_size
    from .test_guided_gpu import ULP
    from .test_guided_host import movable
    results = []
    for ctx, b, lens in keyed:
        front, chi, corr, s = one_corrector(ctx, b)
        k = lens.index(64)
        x, y, sc = (torch.split(t.cpu(), list(lens), 1)[k] for t in (front, chi, s))
        c = type(trio[1])({key: (v.cpu() if isinstance(v, torch.Tensor) else v) for key, v in trio[1].items()})
        mov = movable(c) & torch.isfinite(sc)
        z64 = corrector_noise64(64, 2 ** 40 + 5, 0)
        s2, n2, eps, amp = corr[k].tolist()
        want_s2, want_n2 = float((sc.double()[mov] ** 2).sum()), float((z64[mov] ** 2).sum())
        all_s2 = float((sc.double() ** 2).sum())
        print(f"damaged64 in {lens}: s2 {s2!r} (movable entries: {want_s2!r}, every entry: {all_s2!r}), n2 {n2!r} (restated: {want_n2!r})")
        assert all_s2 > want_s2 * (1 + 1e-6)                      # the sum over every entry is another number
        assert abs(s2 - want_s2) <= 1e-12 * want_s2
        assert abs(n2 - want_n2) <= 2e-5 * float(z64[mov].abs().sum()) + 1e-9
        e32, a32 = step_size(s2, n2, SNR)
        assert abs(eps - float(e32)) <= float(np.spacing(e32)) and abs(amp - float(a32)) <= float(np.spacing(a32))
        f32 = lambda v: torch.as_tensor(float(v), dtype=torch.float32)
        yy = x + f32(eps) * sc
        yy = yy + f32(amp) * z64.float()
        want = torch.where(mov, O.wrap_pi(yy) * c["SC_D_mask"], x)
        assert torch.equal(y[~mov], x[~mov])
        bound = 1e-5 * amp + 4 * ULP
        d = float(wrapped_absdiff(y, want)[mov].max())
        print(f"damaged64 in {lens}: max wrapped |device - restated update| = {d:.3g}, bound {bound:.3g}")
        assert d <= bound
        assert int((wrapped_absdiff(y, x)[mov] > 0.01).sum()) >= 30
        results.append(y)
    assert torch.equal(results[0], results[1])
