"""Clash-guided sampling on the device (pp_sample_guided) against the restatement of tests/test_guided_host.py.

Shapes: L = 24 alone (K = 24 < 32) and one packed batch of (40, 7), (64, 11) and the 33-row complex (33, 107); six steps,
``torch.linspace(1, 0, 7)``, the weights of WEIGHT_SEED; SDE noise restated from the NumPy generator.  The fp32 and fp64 restatement
runs are made once per (complex, mode, pin) and shared.
"""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from .conftest import wrapped_absdiff
from .test_guided_host import (CAP, CASES, ETA_CONST, EXTRA, KEYS, SCALE, SCHED, SEED, cpu, fixed_rows, nudge, reference, rolled,
                               self_distance)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = len(SCHED) - 1
PACK = (CASES[1], CASES[2], EXTRA)             # (40, 7), (64, 11), (33, 107)
ULP = 2.0 ** -21                               # one fp32 ulp of the largest value wrap_pi forms, x + pi in [4, 8)
TWO_PI_F = 6.2831854820251465                  # the period the reverse step's wrap_pi uses (fp32)
ETA_MIX = np.float32([0, SCALE, 0, SCALE, SCALE, 0, SCALE])


@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = SCHED
    return m


def dev_complex(L):
    c = cpu(L).to(DEV)
    c["complex_key"] = KEYS[L]
    c["complex_keys"] = [KEYS[L]]
    return c


@pytest.fixture(scope="module")
def complexes():
    return {L: dev_complex(L) for L in (24, 40, 64, 33)}


def _ctx(model, batch, keys):
    from packppi_amd.lib import Context
    ctx = Context(model._plan, batch)
    ctx.set_rng_keys(keys)
    return ctx


@pytest.fixture(scope="module")
def solo(model, complexes):
    """{L: (ctx, batch)} of every complex alone."""
    return {L: (_ctx(model, c, [KEYS[L]]), c) for L, c in complexes.items()}


@pytest.fixture(scope="module")
def packed(model, complexes):
    from packppi_amd.batch import pack
    pb = pack([complexes[L] for L, _ in PACK])
    return _ctx(model, pb, [KEYS[L] for L, _ in PACK]), pb


def contexts(solo, packed):
    """(name, ctx, batch, lengths) of the two shapes every test runs on."""
    return (("L24", solo[24][0], solo[24][1], (24,)), ("pack137", packed[0], packed[1], tuple(L for L, _ in PACK)))


def split(t, lens, dim=1):
    return torch.split(t, list(lens), dim=dim)


def cat_fixed(lens):
    return torch.cat([fixed_rows(L) for L in lens]).to(DEV)


def cat_rolled(lens):
    return torch.cat([rolled(cpu(L)) for L in lens], 1).to(DEV)


# ---- 1. zero eta ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_zero_eta_is_todays_sampler(mode, solo, packed):
    zero = np.zeros(N + 1, dtype=np.float32)
    for name, ctx, b, lens in contexts(solo, packed):
        init = ctx.add_noise(b.SC_D, 1.0, SEED)
        want = ctx.sample(init, SCHED, mode, seed=SEED)
        got, traj, trace = ctx.sample_guided(init, SCHED, mode, SEED, zero, trajectory=True, want_trace=True)
        assert torch.equal(got, want) and torch.equal(traj[-1], want) and not torch.equal(want, init), name
        assert trace.shape == (len(lens), N + 1) and bool(torch.isnan(trace).all())
        fx, ref = cat_fixed(lens), cat_rolled(lens)
        for fix_mode in ("hold", "renoise"):
            w, wt = ctx.sample_partial(init, ref, fx, SCHED, mode, SEED, fix_mode, trajectory=True)
            g, gt, tr = ctx.sample_guided(init, SCHED, mode, SEED, zero, chi_ref=ref, fixed=fx, fix_mode=fix_mode, trajectory=True,
                                          want_trace=True)
            assert torch.equal(g, w) and torch.equal(gt, wt) and bool(torch.isnan(tr).all()), (name, fix_mode)


# ---- 2. one nudge in isolation ---------------------------------------------------------------------------------------------------------
SCHED2 = SCHED[-2:]


def one_nudge(ctx, b, e, cap, **kw):
    init = ctx.add_noise(b.SC_D, 1.0, SEED)
    chi, traj = ctx.sample_guided(init, SCHED2, "ode", SEED, np.float32([0, e]), cap=cap, trajectory=True, **kw)
    return traj[0], chi


def check_one_nudge(front, chi, lens, e, cap, obst=None):
    """The restated nudge on the device's own state in front of it, complex by complex."""
    worst, n_mov, reach = 0.0, 0, 0.0
    for L, x, y in zip(lens, split(front.cpu(), lens), split(chi.cpu(), lens)):
        want, _, mov, G = nudge(cpu(L), x, e, cap, obst=obst[L] if obst else None)
        assert torch.equal(y[~mov], x[~mov]), L                       # lanes outside the movable set: bit for bit
        worst = max(worst, float(wrapped_absdiff(y, want).max()))
        n_mov += int(mov.sum())
        step = (y.double() - x.double()).abs()[mov]
        reach = max(reach, float(torch.where(step > math.pi, TWO_PI_F - step, step).max()))       # a lane that wrapped moved by the rest
    return worst, n_mov, reach


@pytest.mark.parametrize("cap", [CAP, 1e-3, math.inf])
def test_one_nudge_in_isolation(cap, solo, packed):
    e = 0.05
    for name, ctx, b, lens in contexts(solo, packed):
        front, chi = one_nudge(ctx, b, e, cap)
        worst, n_mov, reach = check_one_nudge(front, chi, lens, e, cap)
        print(f"{name} cap {cap}: max wrapped |device - restated nudge| = {worst:.3g} over {n_mov} movable lanes; largest move {reach:.6g}")
        assert n_mov > 0 and worst <= 2e-6
        if math.isfinite(cap):
            assert reach <= cap + ULP                              # no lane moves farther than the cap plus one ulp
            assert reach >= cap - ULP                              # ... and some lane reaches it
        else:
            assert reach > CAP                                        # without the clamp some lane goes beyond the default cap


def overlapping_obstacles(L, front, n_rows=3, per_row=4):
    from .test_obstacles_host import place_near_terminals
    return place_near_terminals(cpu(L), front, n_rows, per_row, 0.5, 1.2, seed=64 + L, overlap=True)[0]


def install(ctx, lens, obst):
    """The per-complex obstacle sets [M_L, 4] as one set with one range per segment."""
    offs, parts = [0], []
    for L in lens:
        parts.append(obst[L])
        offs.append(offs[-1] + len(obst[L]))
    ctx.set_obstacles(torch.cat(parts).to(DEV), [(a, b - a) for a, b in zip(offs[:-1], offs[1:])])


def test_one_nudge_with_obstacles(solo, packed):
    """The same with a set installed that overlaps side chains at the state in front of the nudge (which does not depend on the set:
    the network does not see it); then test 8: a far-away set and a cleared set change no bit, the set in reach changes the result."""
    e = 0.05
    for name, ctx, b, lens in contexts(solo, packed):
        try:
            front0, plain = one_nudge(ctx, b, e, CAP)
            obst = {L: overlapping_obstacles(L, x) for L, x in zip(lens, split(front0.cpu(), lens))}
            install(ctx, lens, obst)
            front, chi = one_nudge(ctx, b, e, CAP)
            assert torch.equal(front, front0)
            worst, n_mov, _ = check_one_nudge(front, chi, lens, e, CAP, obst)
            moved = float(wrapped_absdiff(chi.cpu(), plain.cpu()).max())
            print(f"{name}: max wrapped |device - restated nudge| with obstacles = {worst:.3g}; the set moves the result by {moved:.3g} rad")
            assert worst <= 2e-6 and moved > 1e-3
            far = {L: o + torch.tensor([1e4, 0, 0, 0]) for L, o in obst.items()}
            install(ctx, lens, far)
            assert torch.equal(one_nudge(ctx, b, e, CAP)[1], plain)
            ctx.set_obstacles(None)
            assert torch.equal(one_nudge(ctx, b, e, CAP)[1], plain)
        finally:
            ctx.set_obstacles(None)


# ---- 3. one guided step, teacher-forced ------------------------------------------------------------------------------------------------
def test_one_guided_step_teacher_forced(solo, packed):
    """For every j the device takes the fp32 restatement's iterate x_j with schedule[j : j + 2] and eta = [eta_j, 0]; the result is
    within 1e-4 rad (the project's figure for pp_sample against the oracle) of the restatement's x_{j+1}."""
    for name, ctx, b, lens in contexts(solo, packed):
        refs = [reference(L, "ode", False, torch.float32) for L in lens]
        worst = 0.0
        for j in range(N):
            xj = torch.cat([r[0] if j == 0 else r[2][j - 1] for r in refs], 1)
            want = torch.cat([r[2][j] for r in refs], 1)
            got = ctx.sample_guided(xj.to(DEV), SCHED[j:j + 2], "ode", SEED, np.float32([ETA_CONST[j], 0]), cap=CAP)
            worst = max(worst, float(wrapped_absdiff(got.cpu(), want).max()))
        print(f"{name}: max wrapped |device step - restated step| over {N} teacher-forced steps = {worst:.3g}")
        assert worst < 1e-4


# ---- 4. free-running -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_free_running_six_steps(mode, pinned, solo, packed):
    """Every chi_traj step and the final chi within twice the restatement's own fp32 <-> fp64 distance (measured here, on the
    reference alone) of the fp32 restatement.  Control: guided and unguided differ by more than 0.1 rad somewhere."""
    for name, ctx, b, lens in contexts(solo, packed):
        refs = [reference(L, mode, pinned, torch.float32) for L in lens]
        init = torch.cat([r[0] for r in refs], 1).to(DEV)
        kw = dict(chi_ref=cat_rolled(lens), fixed=cat_fixed(lens), fix_mode="renoise") if pinned else {}
        chi, traj = ctx.sample_guided(init, SCHED, mode, SEED, ETA_CONST, cap=CAP, trajectory=True, **kw)
        for k, L in enumerate(lens):
            bound = 2 * self_distance(L, mode, pinned)
            got = [split(t.cpu(), lens)[k] for t in traj] + [split(chi.cpu(), lens)[k]]
            want = refs[k][2] + [refs[k][1]]
            d = max(float(wrapped_absdiff(g, w).max()) for g, w in zip(got, want))
            print(f"{name} L = {L} {mode} pinned = {pinned}: max wrapped |device - fp32 restatement| = {d:.3g}, "
                  f"twice the restatement's fp32 <-> fp64 distance = {bound:.3g}")
            assert d <= bound, (L, d, bound)
        zero = np.zeros(N + 1, dtype=np.float32)
        plain = ctx.sample_guided(init, SCHED, mode, SEED, zero, **kw)
        gap = float(wrapped_absdiff(chi.cpu(), plain.cpu()).max())
        print(f"{name} {mode} pinned = {pinned}: max wrapped |guided - unguided| = {gap:.3g}")
        assert gap > 0.1


# ---- 5. trace ------------------------------------------------------------------------------------------------------------------------
def test_trace(solo, packed):
    """clash_trace[s][j] against the restated mean clash at the device's own state in front of nudge j (the init, then chi_traj[j - 1]):
    within 5e-5, the project's figure for loss values; NaN exactly where eta is 0."""
    for name, ctx, b, lens in contexts(solo, packed):
        init = ctx.add_noise(b.SC_D, 1.0, SEED)
        chi, traj, trace = ctx.sample_guided(init, SCHED, "ode", SEED, ETA_MIX, cap=CAP, trajectory=True, want_trace=True)
        trace = trace.cpu()
        assert trace.dtype == torch.float64 and trace.shape == (len(lens), N + 1)
        assert torch.equal(torch.isnan(trace), torch.from_numpy(ETA_MIX == 0).expand(len(lens), -1))
        worst = 0.0
        for j in np.nonzero(ETA_MIX)[0]:
            front = (init if j == 0 else traj[j - 1]).cpu()
            for k, (L, x) in enumerate(zip(lens, split(front, lens))):
                worst = max(worst, abs(nudge(cpu(L), x, ETA_MIX[j], CAP)[1] - float(trace[k, j])))
        print(f"{name}: max |trace - restated mean clash| = {worst:.3g}; trace {trace[0].tolist()}")
        assert worst < 5e-5


# ---- 6. packing invariance -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,pinned", [("sde", False), ("ode", True)])
def test_packing_invariance(mode, pinned, solo, packed):
    ctx, pb = packed
    lens = tuple(L for L, _ in PACK)

    def run(c, b, ls):
        init = c.add_noise(b.SC_D, 1.0, SEED)
        kw = dict(chi_ref=cat_rolled(ls), fixed=cat_fixed(ls), fix_mode="renoise") if pinned else {}
        return c.sample_guided(init, SCHED, mode, SEED, ETA_MIX, cap=CAP, trajectory=True, want_trace=True, **kw)

    chi, traj, trace = run(ctx, pb, lens)
    again = run(ctx, pb, lens)
    assert all(torch.equal(a, b) for a, b in zip((chi, traj, trace[:, ETA_MIX != 0]), (again[0], again[1], again[2][:, ETA_MIX != 0])))
    for k, L in enumerate(lens):
        c1, t1, r1 = run(solo[L][0], solo[L][1], (L,))
        assert torch.isfinite(c1).all()
        assert torch.equal(c1, split(chi, lens)[k]), L
        assert torch.equal(t1, split(traj, lens, dim=2)[k]), L
        assert torch.equal(r1[0, ETA_MIX != 0], trace[k, ETA_MIX != 0]), L


# ---- 7. pin ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["ode", "sde"])
def test_pin(mode, solo, packed):
    for name, ctx, b, lens in contexts(solo, packed):
        fx, ref = cat_fixed(lens), cat_rolled(lens)
        init = ctx.add_noise(torch.where(fx.reshape(1, -1, 1), ref, b.SC_D), 1.0, SEED)
        for fix_mode in ("hold", "renoise"):
            start = torch.where(fx.reshape(1, -1, 1), ref, init) if fix_mode == "hold" else init
            chi, traj = ctx.sample_guided(start, SCHED, mode, SEED, ETA_CONST, cap=CAP, chi_ref=ref, fixed=fx, fix_mode=fix_mode,
                                          trajectory=True)
            assert torch.equal(chi[0, fx], ref[0, fx]) and not torch.equal(chi[0, ~fx], ref[0, ~fx]), (name, fix_mode)
            if fix_mode == "hold":
                assert all(torch.equal(t[0, fx], ref[0, fx]) for t in traj)
        free = torch.zeros_like(fx)
        a = ctx.sample_guided(init, SCHED, mode, SEED, ETA_CONST, cap=CAP, chi_ref=ref, fixed=free, fix_mode="renoise")
        assert torch.equal(a, ctx.sample_guided(init, SCHED, mode, SEED, ETA_CONST, cap=CAP)), name


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals(model, solo, complexes, weights):
    from packppi_amd import lib as L
    from packppi_amd.functional import _ctx_for
    from packppi_amd.lib import Context, Plan
    lib = L.load()
    ctx, b = solo[24]
    ctx.plan.set_clash_params(12.0, 0.5)
    chi = ctx.add_noise(b.SC_D, 1.0, SEED)
    ref = rolled(cpu(24)).to(DEV).contiguous()
    fx = fixed_rows(24).to(DEV).to(torch.uint8).contiguous()
    sched = np.ascontiguousarray(SCHED.numpy(), dtype=np.float32)
    eta = np.ascontiguousarray(ETA_CONST)
    f = ctypes.c_float

    def call(handle=ctx.handle, chi_p=chi.data_ptr(), ref_p=None, fx_p=None, sch=sched.ctypes.data, et=eta, cap=0.1, mode=0):
        return lib.pp_sample_guided(handle, chi_p, ref_p, fx_p, 1, sch, len(sched), mode, SEED,
                                    et.ctypes.data if et is not None else None, f(cap), None, None, None)

    def refused(word, **kw):
        assert call(**kw) == 1, (word, kw)
        msg = lib.pp_last_error().decode()
        assert "pp_sample_guided" in msg and word in msg, (word, msg)

    refused("ctx", handle=None)
    refused("chi", chi_p=None)
    refused("schedule", sch=None)
    refused("eta", et=None)
    refused("chi_ref and fixed", ref_p=ref.data_ptr())
    refused("chi_ref and fixed", fx_p=fx.data_ptr())
    for bad in (-0.01, math.nan, math.inf):
        e = eta.copy()
        e[3] = bad
        refused("eta[3]", et=e)
    for bad in (0.0, -0.1, math.nan):
        refused("cap", cap=bad)
    assert call(cap=math.inf, et=np.zeros_like(eta)) == 0                  # INFINITY is allowed: no clamp
    # no clash parameters yet: a fresh plan
    plan = Plan(weights, torch.device(DEV))
    fresh = Context(plan, b)
    refused("pp_plan_set_clash_params", handle=fresh.handle)
    # a padded B > 1 context
    two = type(b)(b)
    for k, v in b.items():
        if isinstance(v, torch.Tensor) and v.dim() >= 2 and v.shape[0] == 1:
            two[k] = torch.cat([v, v], 0).contiguous()
    two["num_proteins"] = 2
    padded = Context(ctx.plan, two)
    chi2 = torch.cat([chi, chi], 0).contiguous()
    refused("padded", handle=padded.handle, chi_p=chi2.data_ptr())
    # a geometry-only plan (its batches carry atom_mask and residue_index, not the network's tensors)
    geo = _ctx_for(b)
    geo.plan.set_clash_params(12.0, 0.5)
    refused("geometry-only", handle=geo.handle)
    # a batch without atom_mask / residue_index / the periodic masks can only be prepared on a geometry-only plan, which is refused
    # first: the three messages are reached through the same checks in that order (pp_api.hip)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="together"):
        ctx.sample_guided(chi, SCHED, "ode", SEED, eta, chi_ref=ref)
    with pytest.raises(ValueError, match="entries"):
        ctx.sample_guided(chi, SCHED, "ode", SEED, eta[:-1])


# ---- 10. the Python layers ---------------------------------------------------------------------------------------------------------------
def test_sampling_equals_the_context_call(model, solo, complexes):
    ctx, b = solo[40]
    g = dict(scale=0.05, kind="constant", cap=0.2)
    eta = np.full(N + 1, 0.05, dtype=np.float32)
    init = ctx.add_noise(b.SC_D, 1.0, 9)
    want, wt, wr = ctx.sample_guided(init, SCHED, "ode", 9, eta, cap=0.2, trajectory=True, want_trace=True)
    got, gt, gr = model.sampling(b, seed=9, guide=g, return_trajectory=True)
    assert torch.equal(got, want) and torch.equal(gt, wt) and torch.equal(gr, wr)
    assert torch.equal(model.sampling(b, seed=9, guide=eta.tolist()), model.sampling(b, seed=9, guide=dict(scale=0.05, kind="constant")))
    assert not torch.equal(got, model.sampling(b, seed=9))
    fx = fixed_rows(40).reshape(1, -1).to(DEV)
    out = model.repack(b, fx, seed=9, guide=g)
    assert torch.equal(out[fx], b.SC_D[fx]) and not torch.equal(out, model.repack(b, fx, seed=9))
    # use_proximal runs behind it, as today
    prox = model.sampling(b, seed=9, guide=g, use_proximal=True)
    assert prox.shape == got.shape and torch.isfinite(prox).all()


def test_ensemble_decoys_are_the_complex_alone(model, complexes):
    from packppi_amd.batch import decoy_key, unpack
    b = complexes[40]
    out = model.sample_ensemble(b, 3, seed=9, guide=0.05, return_all=True)
    chi, pk = out["decoys"]
    for d, part in enumerate(unpack(pk, chi)):
        alone = type(b)(b)
        alone["complex_key"] = decoy_key(KEYS[40], d)
        alone["complex_keys"] = [decoy_key(KEYS[40], d)]
        assert torch.equal(part, model.sampling(alone, seed=9, guide=0.05)), d
    assert not torch.equal(chi, model.sample_ensemble(b, 3, seed=9, return_all=True)["decoys"][0])


def test_mutate_keeps_unshelled_rows(model):
    from packppi_amd import constants as rc
    from packppi_amd import synth
    protein = synth.make_complex(64, 11)
    i = int(np.nonzero(np.asarray(protein["aaindex"]) != rc.restype_order["A"])[0][5])
    wt = rc.restypes[int(protein["aaindex"][i])]
    mut = f"{wt}{protein['chain_id'][i]}{int(protein['residue_index'][i])}A"
    r = model.mutate([(protein, mut)], seed=4, guide=dict(scale=0.05, kind="constant"), log=lambda *a: None)[0]
    plain = model.mutate([(protein, mut)], seed=4, log=lambda *a: None)[0]
    keep = ~r["shell"]
    assert keep.any() and r["shell"].any()
    assert torch.equal(r["SC_D"][keep], r["batch"]["SC_D"][keep])
    assert torch.equal(r["shell"], plain["shell"]) and not torch.equal(r["SC_D"], plain["SC_D"])


def test_eval_diffusion_cli(tmp_path, capsys):
    """--guide writes guide.csv with n_schedule lines per complex and prints the traced clash; the run without the flag leaves the
    files of the golden run of tests/test_hip_cli.py with the bytes the parent commit wrote (tests/golden/g21_cli_parent.txt holds the
    SHA-256 of the parent's structure.pdb for exactly these arguments)."""
    import hashlib
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.pdb_io import to_pdb
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    base = ["--input", str(pdb), "--molprobity_clash_loc", "/nonexistent", "--device", "cuda", "--random_weights", "3", "--steps", "10",
            "--seed", "5", "--use_proximal"]
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "plain")])
    capsys.readouterr()
    assert sorted(os.listdir(tmp_path / "plain")) == ["structure.pdb"]
    golden = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_cli_parent.txt")).read().split()
    assert hashlib.sha256((tmp_path / "plain" / "structure.pdb").read_bytes()).hexdigest() == golden[0]
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "guided"), "--guide", "0.05", "--guide_schedule", "constant"])
    text = capsys.readouterr().out
    assert sorted(os.listdir(tmp_path / "guided")) == ["guide.csv", "structure.pdb"]
    lines = (tmp_path / "guided" / "guide.csv").read_text().splitlines()
    assert lines[0] == "complex,nudge_point,t,eta,mean_clash" and len(lines) - 1 == 11                # n_schedule = steps + 1
    assert all(ln.split(",")[4] != "" for ln in lines[1:]) and "guide: mean clash in front of the first nudge" in text
    assert (tmp_path / "guided" / "structure.pdb").read_bytes() != (tmp_path / "plain" / "structure.pdb").read_bytes()
