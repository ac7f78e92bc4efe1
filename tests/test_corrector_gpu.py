"""Predictor-corrector sampling on the device (pp_sample_corrected) against the restatement of
tests/test_corrector_host.py.

Shapes: L = 24 alone (K = 24 < 32), one packed batch of (40, 7), (64, 11) and the 33-row complex (33, 107), and a padded B = 2 batch
of two L = 24 complexes; ``torch.linspace(1, 0, 7)`` (six steps), its two-entry tail (one corrector in isolation) and its four-entry
tail (the three-step whole run); the weights of WEIGHT_SEED.
"""
import math

import numpy as np
import pytest
import torch

from .conftest import wrapped_absdiff
from .test_corrector_host import SCHED2, SCHED4, SNR, SNR4, corrector_noise64, reference4, self_distance4, step_size
from .test_guided_gpu import (DEV, N, PACK, ULP, _ctx, cat_fixed, cat_rolled, complexes, contexts, model, packed, solo,  # noqa: F401
                              split)
from .test_guided_host import CAP, ETA_CONST, KEYS, SCHED, SEED, complex_cpu, cpu, fixed_rows, movable, nudge

pytestmark = pytest.mark.gpu
ONE = np.float32([SNR])
LENS_PACK = tuple(L for L, _ in PACK)


def snr6():
    from packppi_amd.schedule import corrector_snr
    return corrector_snr(SCHED, SNR)


def isnan_all(t):
    return bool(torch.isnan(t).all())


# ---- 1. zero snr ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_zero_snr_is_todays_sampler(mode, solo, packed):
    zero = np.zeros(N, dtype=np.float32)
    for name, ctx, b, lens in contexts(solo, packed):
        init = ctx.add_noise(b.SC_D, 1.0, SEED)
        want = ctx.sample(init, SCHED, mode, seed=SEED)
        got, traj, corr = ctx.sample_corrected(init, SCHED, mode, SEED, zero, trajectory=True, want_corr=True)
        assert torch.equal(got, want) and torch.equal(traj[-1], want) and not torch.equal(want, init), name
        assert corr.shape == (len(lens), N, 4) and corr.dtype == torch.float64 and isnan_all(corr)
        fx, ref = cat_fixed(lens), cat_rolled(lens)
        for fix_mode in ("hold", "renoise"):
            w, wt = ctx.sample_partial(init, ref, fx, SCHED, mode, SEED, fix_mode, trajectory=True)
            g, gt, cr = ctx.sample_corrected(init, SCHED, mode, SEED, zero, chi_ref=ref, fixed=fx, fix_mode=fix_mode, trajectory=True,
                                             want_corr=True)
            assert torch.equal(g, w) and torch.equal(gt, wt) and isnan_all(cr), (name, fix_mode)
        w, wt, wr = ctx.sample_guided(init, SCHED, mode, SEED, ETA_CONST, cap=CAP, trajectory=True, want_trace=True)
        g, gt, gr, cr = ctx.sample_corrected(init, SCHED, mode, SEED, zero, eta=ETA_CONST, cap=CAP, trajectory=True, want_trace=True,
                                             want_corr=True)
        assert torch.equal(g, w) and torch.equal(gt, wt) and torch.equal(gr, wr) and isnan_all(cr), name


# ---- 2. one corrector in isolation ----------------------------------------------------------------------------------------------------
def one_corrector(ctx, b, **kw):
    """(front = the state in front of the corrector, the result, the trace rows [n_seg, 4], the device's score at front)."""
    init = ctx.add_noise(b.SC_D, 1.0, SEED)
    if "fixed" in kw and kw.get("fix_mode") == "hold":
        init = torch.where(kw["fixed"].reshape(1, -1, 1) != 0, kw["chi_ref"], init)
    chi, traj, corr = ctx.sample_corrected(init, SCHED2, "ode", SEED, ONE, trajectory=True, want_corr=True, **kw)
    return traj[0], chi, corr[:, 0].cpu(), ctx.score(traj[0], float(SCHED2[1]))[0]


def check_one_corrector(front, chi, corr, s, lens, fixed=None, min_moved=30):
    """Test 2's bounds, complex by complex; returns the worst wrapped |device - restated update| in units of its bound."""
    worst = 0.0
    for k, (L, x, y, sc) in enumerate(zip(lens, split(front.cpu(), lens), split(chi.cpu(), lens), split(s.cpu(), lens))):
        b = cpu(L)
        fx = fixed[k] if fixed is not None else None
        mov = movable(b, fx) & torch.isfinite(sc)
        z64 = corrector_noise64(L, KEYS[L], 0)
        s2, n2, eps, amp = corr[k].tolist()
        want_s2 = float((sc.double()[mov] ** 2).sum())
        want_n2 = float((z64[mov] ** 2).sum())
        print(f"L = {L}: s2 {s2!r} (fp64 sum of the device's score^2: {want_s2!r}), n2 {n2!r} (restated: {want_n2!r}), eps {eps!r}, amp {amp!r}, "
              f"{int(mov.sum())} movable entries")
        assert abs(s2 - want_s2) <= 1e-12 * want_s2, L
        assert abs(n2 - want_n2) <= 2e-5 * float(z64[mov].abs().sum()) + 1e-9, L
        e32, a32 = step_size(s2, n2, SNR)                       # the formula on the device's own s2, n2
        assert abs(eps - float(e32)) <= float(np.spacing(e32)) and abs(amp - float(a32)) <= float(np.spacing(a32)), L
        assert 0.01 < eps < 1, L                                 # not a degenerate input
        # the update restated in fp32 from the device's eps, amp, s and the restated z
        f32 = lambda v: torch.as_tensor(float(v), dtype=torch.float32)
        yy = x + f32(eps) * sc
        yy = yy + f32(amp) * z64.float()
        from oracle import ref_cpu as O
        want = torch.where(mov, O.wrap_pi(yy) * b["SC_D_mask"], x)
        assert torch.equal(y[~mov], x[~mov]), L                  # entries outside the movable set: bit for bit
        bound = 1e-5 * amp + 4 * ULP
        d = float(wrapped_absdiff(y, want)[mov].max())
        print(f"L = {L}: max wrapped |device - restated update| = {d:.3g}, bound {bound:.3g}")
        assert d <= bound, (L, d, bound)
        worst = max(worst, d / bound)
        moved = int((wrapped_absdiff(y, x)[mov] > 0.01).sum())
        assert moved >= (min_moved if min_moved is not None else (int(mov.sum()) + 1) // 2), (L, moved)
    return worst


def test_one_corrector_in_isolation(solo, packed):
    for name, ctx, b, lens in contexts(solo, packed):
        front, chi, corr, s = one_corrector(ctx, b)
        worst = check_one_corrector(front, chi, corr, s, lens)
        print(f"{name}: worst update error = {worst:.3g} of its bound")


# ---- 3. packing invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_packing_invariance(mode, solo, packed, model):
    snr = snr6()

    def run(c, b):
        init = c.add_noise(b.SC_D, 1.0, SEED)
        return c.sample_corrected(init, SCHED, mode, SEED, snr, trajectory=True, want_corr=True)

    ctx, pb = packed
    chi, traj, corr = run(ctx, pb)
    assert torch.isfinite(corr[:, snr != 0]).all() and isnan_all(corr[:, snr == 0])
    for k, L in enumerate(LENS_PACK):
        c1, t1, r1 = run(*solo[L])
        assert torch.isfinite(c1).all()
        assert torch.equal(c1, split(chi, LENS_PACK)[k]), L
        assert torch.equal(t1, split(traj, LENS_PACK, dim=2)[k]), L
        assert torch.equal(r1[0, snr != 0], corr[k, snr != 0]), L
    # a padded B = 2 batch of two L = 24 complexes
    second = complex_cpu(24, 6).to(DEV)
    first = solo[24][1]
    pad = type(first)(first)
    for key, v in first.items():
        if isinstance(v, torch.Tensor) and v.dim() >= 2 and v.shape[0] == 1:
            pad[key] = torch.cat([v, second[key]], 0)
    pad["num_proteins"] = 2
    pad.pop("complex_key", None)
    keys = [KEYS[24], KEYS[24] + 1]
    pctx = _ctx(model, pad, keys)
    assert not pctx.packed and pctx.B == 2
    chi, traj, corr = run(pctx, pad)
    for k, (b1, key) in enumerate(zip((first, second), keys)):
        c1, t1, r1 = run(_ctx(model, b1, [key]), b1)
        assert torch.equal(c1[0], chi[k]) and torch.equal(t1[:, 0], traj[:, k]) and torch.equal(r1[0, snr != 0], corr[k, snr != 0]), k
    assert not torch.equal(chi[0], chi[1])


def test_every_corrector_of_a_run_scores_like_pp_score(solo, packed):
    """Six steps, a corrector behind the first five: every trace row's s2 is the fp64 sum, within 1e-12, of the squares of
    ctx.score(chi_traj[j], schedule[j + 1]) over the movable entries -- the corrector's evaluation is pp_score's behind any step,
    not only behind the last one."""
    snr = snr6()
    for name, ctx, b, lens in contexts(solo, packed):
        init = ctx.add_noise(b.SC_D, 1.0, SEED)
        chi, traj, corr = ctx.sample_corrected(init, SCHED, "sde", SEED, snr, trajectory=True, want_corr=True)
        for j in np.nonzero(snr)[0]:
            s = ctx.score(traj[j], float(SCHED[j + 1]))[0].cpu()
            for k, (L, sc) in enumerate(zip(lens, split(s, lens))):
                want = float((sc.double()[movable(cpu(L)) & torch.isfinite(sc)] ** 2).sum())
                assert abs(float(corr[k, j, 0]) - want) <= 1e-12 * want and 0.01 < float(corr[k, j, 2]) < 1, (name, j, L)


# ---- 4. pin -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fix_mode", ["hold", "renoise"])
def test_pin(fix_mode, solo, packed):
    for name, ctx, b, lens in contexts(solo, packed):
        fx, ref = cat_fixed(lens), cat_rolled(lens)
        kw = dict(chi_ref=ref, fixed=fx, fix_mode=fix_mode)
        init = ctx.add_noise(torch.where(fx.reshape(1, -1, 1), ref, b.SC_D), 1.0, SEED)
        if fix_mode == "hold":
            init = torch.where(fx.reshape(1, -1, 1), ref, init)
        for mode in ("ode", "sde"):
            chi = ctx.sample_corrected(init, SCHED, mode, SEED, snr6(), **kw)
            assert torch.equal(chi[0, fx], ref[0, fx]) and torch.isfinite(chi).all(), (name, mode)
            assert not torch.equal(chi, ctx.sample_partial(init, ref, fx, SCHED, mode, SEED, fix_mode))
        # in isolation: only the free movable entries are counted, no fixed row moves
        front, chi, corr, s = one_corrector(ctx, b, **kw)
        assert torch.equal(front[0, fx], chi[0, fx]) and torch.equal(chi[0, fx], ref[0, fx])
        # (two thirds of the rows are fixed: L = 24 keeps 20 movable entries, so "moved" asks for half of them instead of 30)
        check_one_corrector(front, chi, corr, s, lens, fixed=[fixed_rows(L) for L in lens], min_moved=None)
        for k, (L, sc) in enumerate(zip(lens, split(s.cpu(), lens))):
            everything = float((sc.double()[movable(cpu(L))] ** 2).sum())
            assert abs(float(corr[k, 0]) - everything) > 0.01 * everything, L


# ---- 5. a segment without a corrector ---------------------------------------------------------------------------------------------------
def test_a_segment_without_a_corrector(solo, packed):
    ctx, pb = packed
    fixed = {40: fixed_rows(40), 64: fixed_rows(64), 33: torch.ones(33, dtype=torch.bool)}
    fx = torch.cat([fixed[L] for L in LENS_PACK]).to(DEV)
    ref = cat_rolled(LENS_PACK)
    snr = snr6()

    def run(c, b, f, r):
        init = c.add_noise(torch.where(f.reshape(1, -1, 1), r, b.SC_D), 1.0, SEED)
        return c.sample_corrected(init, SCHED, "sde", SEED, snr, chi_ref=r, fixed=f, trajectory=True, want_corr=True)

    chi, traj, corr = run(ctx, pb, fx, ref)
    assert isnan_all(corr[2]) and torch.isfinite(corr[:2, snr != 0]).all()
    part = split(chi, LENS_PACK)[2]
    assert torch.equal(part, split(ref, LENS_PACK)[2]) and torch.equal(part, split(traj[-1], LENS_PACK)[2])
    for k, L in enumerate(LENS_PACK):
        c1, t1, r1 = run(solo[L][0], solo[L][1], fixed[L].to(DEV), split(ref, LENS_PACK)[k].contiguous())
        assert torch.equal(c1, split(chi, LENS_PACK)[k]) and torch.equal(t1, split(traj, LENS_PACK, dim=2)[k]), L
        assert torch.equal(torch.isnan(r1[0]), torch.isnan(corr[k])) and torch.equal(r1[0][~torch.isnan(r1[0])], corr[k][~torch.isnan(corr[k])]), L
    # the fully fixed complex alone: the corrector never touched it -- every trajectory step is the pinned step's own
    ref33, fx33 = split(ref, LENS_PACK)[2].contiguous(), fixed[33].to(DEV)
    c33, t33, r33 = run(solo[33][0], solo[33][1], fx33, ref33)
    w33, wt33 = solo[33][0].sample_partial(solo[33][0].add_noise(ref33, 1.0, SEED), ref33, fx33, SCHED, "sde", SEED, "renoise",
                                           trajectory=True)
    assert torch.equal(c33, w33) and torch.equal(t33, wt33) and isnan_all(r33)


# ---- 6. the whole run against the restatement -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [24, 40])
def test_whole_run_against_the_restatement(L, solo):
    """Three steps (the four-entry tail of the schedule), SDE, a corrector behind steps 0 and 1: every trajectory step and the final
    angles against the fp32 restatement, within max(1e-5, 4 x the restatement's own fp32 <-> fp64 wrapped distance), off the entries
    whose two restatement precisions are more than 0.1 rad apart (at most 2 %; on these two cases none: measured on the CPU by
    tests/test_corrector_host.py::test_whole_run_cases_are_within_the_flip_cap, so three steps were kept)."""
    ctx, b = solo[L]
    init, want_chi, want_traj, want_corr = reference4(L, torch.float32)
    own, frac, flipped = self_distance4(L)
    assert frac <= 0.02
    bound = max(1e-5, 4 * own)
    chi, traj, corr = ctx.sample_corrected(init.to(DEV), SCHED4, "sde", SEED, SNR4, trajectory=True, want_corr=True)
    d = max(float(wrapped_absdiff(g.cpu(), w)[~flipped].max()) for g, w in zip(list(traj) + [chi], want_traj + [want_chi]))
    eps = corr[0, :, 2].cpu().tolist()
    print(f"L = {L}: max wrapped |device - fp32 restatement| = {d:.3g}; bound {bound:.3g} (the restatement's fp32 <-> fp64 distance "
          f"{own:.3g}, flipped fraction {frac:.4f}); eps device {eps}, restated {[r[2] for r in want_corr]}")
    assert all(0.01 < e < 1 for e in eps[:2]) and math.isnan(eps[2])
    assert d <= bound, (L, d, bound)


# ---- 7. guide and corrector together --------------------------------------------------------------------------------------------------
def test_guide_and_corrector_order(solo):
    """L = 24 with ETA_CONST's step size.  One reverse step (the tail of the schedule), a corrector behind it and a nudge behind that:
    given traj[0], the restated corrector (test 2's bounds, on the device's own score and step size) gives the state in front of the
    nudge, and the restated nudge from there gives the returned state within the guide test's own nudge bound, 2e-6.  Inside a run
    the next evaluation embeds exactly that state: a two-step run is bit-equal to its two halves chained."""
    ctx, b = solo[24]
    init = ctx.add_noise(b.SC_D, 1.0, SEED)
    eta = np.float32([0, ETA_CONST[-1]])
    chi, traj, corr = ctx.sample_corrected(init, SCHED2, "ode", SEED, ONE, eta=eta, cap=CAP, trajectory=True, want_corr=True)
    only, traj1, corr1 = ctx.sample_corrected(init, SCHED2, "ode", SEED, ONE, trajectory=True, want_corr=True)
    assert torch.equal(traj, traj1) and torch.equal(corr, corr1)                  # the nudge sits behind the corrector
    check_one_corrector(traj[0], only, corr[:, 0].cpu(), ctx.score(traj[0], float(SCHED2[1]))[0], (24,))
    d = float(wrapped_absdiff(chi.cpu(), nudge(cpu(24), only.cpu(), eta[1], CAP)[0]).max())
    print(f"nudge behind the corrector: max wrapped |device - restated nudge| = {d:.3g} (bound 2e-6)")
    assert d <= 2e-6 and not torch.equal(chi, only)
    sn2, eta3 = np.float32([SNR, 0]), np.float32([0, ETA_CONST[1], 0])
    whole, wt = ctx.sample_corrected(init, SCHED[-3:], "ode", SEED, sn2, eta=eta3, cap=CAP, trajectory=True)
    half, ht = ctx.sample_corrected(init, SCHED[-3:-1], "ode", SEED, ONE, eta=eta3[:2], cap=CAP, trajectory=True)
    rest = ctx.sample(half, SCHED[-2:], "ode", seed=SEED)
    assert torch.equal(wt[0], ht[0]) and not torch.equal(half, ht[0]) and torch.equal(whole, rest)


# ---- 8. ensembles -----------------------------------------------------------------------------------------------------------------------
def test_ensemble_decoys_are_the_complex_alone(model, complexes):
    from packppi_amd.batch import decoy_key, unpack
    b = complexes[24]
    out = model.sample_ensemble(b, 2, seed=9, corrector=SNR, return_all=True)
    chi, pk = out["decoys"]
    for d, part in enumerate(unpack(pk, chi)):
        alone = type(b)(b)
        alone["complex_key"] = decoy_key(KEYS[24], d)
        alone["complex_keys"] = [decoy_key(KEYS[24], d)]
        assert torch.equal(part, model.sampling(alone, seed=9, corrector=SNR)), d
    assert not torch.equal(chi, model.sample_ensemble(b, 2, seed=9, return_all=True)["decoys"][0])
    # sampling(return_trajectory=True, corrector=) ends with the corrector trace; the module keeps it for the command lines on request
    got, traj, corr = model.sampling(b, seed=9, corrector=SNR, return_trajectory=True)
    assert corr.shape == (1, N, 4) and torch.isfinite(corr[0, :-1]).all() and isnan_all(corr[0, -1]) and traj.shape[0] == N
    assert torch.equal(got, model.sampling(b, seed=9, corrector=SNR))


# ---- the C entry's refusals -------------------------------------------------------------------------------------------------------------
def test_export_refusals(solo):
    ctx, b = solo[24]
    init = ctx.add_noise(b.SC_D, 1.0, SEED)
    ref = cat_rolled((24,))
    for bad in (-0.1, math.nan, math.inf):
        with pytest.raises(RuntimeError, match="snr\\[1\\] must be finite"):
            ctx.sample_corrected(init, SCHED, "ode", SEED, np.float32([0.1, bad, 0, 0, 0, 0]))
    with pytest.raises(ValueError, match="entries"):
        ctx.sample_corrected(init, SCHED, "ode", SEED, np.float32([0.1] * 7))
    with pytest.raises(ValueError, match="go together"):
        ctx.sample_corrected(init, SCHED, "ode", SEED, snr6(), chi_ref=ref)
    with pytest.raises(RuntimeError, match="distinct"):
        _same_buffer(ctx, init)
    with pytest.raises(RuntimeError, match="eta\\[0\\] must be finite"):
        ctx.sample_corrected(init, SCHED, "ode", SEED, snr6(), eta=np.float32([-1] + [0] * 6))


def _same_buffer(ctx, init):
    """pp_sample_corrected with chi_ref == chi, through the raw binding (Context.sample_corrected clones chi)."""
    from packppi_amd.lib import _check, _stream, load
    sched, snr = np.ascontiguousarray(SCHED.numpy(), dtype=np.float32), snr6()
    chi, fx = init.clone(), cat_fixed((24,)).to(torch.uint8)
    _check(load().pp_sample_corrected(ctx.handle, chi.data_ptr(), chi.data_ptr(), fx.data_ptr(), 1, sched.ctypes.data, len(sched), 0, 1,
                                      snr.ctypes.data, None, 0.1, None, None, None, _stream(ctx.plan.device)), "pp_sample_corrected")
