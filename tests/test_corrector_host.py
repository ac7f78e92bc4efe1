"""Predictor-corrector sampling: the restatement of its definition, and what can be checked without a GPU.

The restatement is composed from the oracle's pieces -- ``network``, ``reverse_step``, ``wrap_pi``, ``encode_static`` --, the guide's
``nudge`` and ``movable`` (tests/test_guided_host.py), the NumPy generator of tests/test_seeded_noise.py at counter step 2^20 + j and
the definition: the corrector and the loop around it, nothing more.  It computes in the dtype it is given, so the same code is the
fp32 reference of the GPU tests and the fp64 run their bounds are measured against.  tests/test_corrector_gpu.py imports it.
"""
import ctypes
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O

from .conftest import wrapped_absdiff
from .test_guided_host import (CAP, ETA_CONST, KEYS, SCHED, SEED, _Probe, complex_cpu, cpu, fixed_rows, guided_run, initial_state,
                               movable, noised, nudge, rolled, sd64, seeded_noise, weights_cpu)
from .test_obstacles_host import cast
from .test_seeded_noise import normals64, words

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SNR = 0.16
CORR_STEP = 2 ** 20                    # the corrector behind reverse step j draws at counter step 2^20 + j
SCHED2 = SCHED[-2:]
SCHED4 = SCHED[-4:]                    # the three-step run of the whole-run test: t = 1/2, 1/3, 1/6, 0
SNR4 = np.float32([SNR, SNR, 0])       # ... with a corrector behind steps 0 and 1


# ---- the restatement -----------------------------------------------------------------------------------------------------------------
def corrector_noise64(L, key, j):
    """fp64 [1, L, 4]: the corrector's N(0,1) draws behind reverse step j (words 0 and 1 of the counter at step 2^20 + j)."""
    return torch.from_numpy(normals64(words(SEED, (L,), (key,), CORR_STEP + j))[0]).reshape(1, L, 4)


def step_size(s2, n2, snr):
    """(eps, amp) as fp32 numbers from the two fp64 norms: the definition's two casts."""
    with np.errstate(all="ignore"):
        snr = float(np.float32(snr))
        eps = np.float32(np.float64(2.0) * snr * snr * np.float64(n2) / np.float64(s2))
        amp = np.float32(np.sqrt(2.0 * np.float64(eps)))
    return eps, amp


def correct(b, x, s, z64, snr, fixed=None):
    """One corrector at ``x`` [1, L, 4] with the score ``s``, both in x's dtype; z64 the fp64 draws (rounded to fp32 first in an
    fp32 run, as the device's normal is an fp32 number).  -> (x', (s2, n2, eps, amp) or four NaN, movable-and-finite mask)."""
    dt = x.dtype
    z = z64.to(dt)
    mov = movable(b, fixed) & torch.isfinite(s)
    s2 = float((s.double()[mov] ** 2).sum())
    n2 = float((z.double()[mov] ** 2).sum())
    eps, amp = step_size(s2, n2, snr)
    if not bool(mov.any()) or s2 == 0 or not (np.isfinite(eps) and np.isfinite(amp)):
        return x, (math.nan,) * 4, mov
    y = x + torch.as_tensor(float(eps), dtype=dt) * s
    y = y + torch.as_tensor(float(amp), dtype=dt) * z
    y = O.wrap_pi(y) * b["SC_D_mask"].to(dt)
    return torch.where(mov, y, x), (s2, n2, float(eps), float(amp)), mov


def corrected_run(sd, b, init, snr, eta=None, cap=CAP, mode="ode", key=0, fixed=None, ref=None, fix_mode="renoise", sched=SCHED):
    """The corrected loop in the dtype of ``b`` / ``sd`` / ``init``: (chi, [chi_traj: in front of each corrector], [corr rows])."""
    dt = init.dtype
    L = init.shape[1]
    n = len(sched) - 1
    m1, m2 = b["chi_1pi_periodic_mask"].reshape(-1, 4), b["chi_2pi_periodic_mask"].reshape(-1, 4)
    scm = b["SC_D_mask"].reshape(-1, 4).to(dt)
    static = O.encode_static(sd, b)
    x, traj, corr = init.clone(), [], []
    if eta is not None and eta[0] != 0:
        x = nudge(b, x, eta[0], cap, fixed)[0]
    for j in range(n):
        time, dtm = sched[j].to(dt), (sched[j] - sched[j + 1]).to(dt)
        score, _ = O.network(sd, b, x, time.repeat_interleave(L), static)
        score, y = score.reshape(-1, 4), x.reshape(-1, 4)
        z = seeded_noise(L, key, j).to(dt) if (mode == "sde" or fixed is not None) else (None, None)
        y = O.reverse_step(y, score, time, dtm, m1, mode, z[0])
        y = O.reverse_step(y, score, time, dtm, m2, mode, z[1])
        y = O.wrap_pi(y) * scm
        if fixed is not None:
            xr = ref.reshape(-1, 4).to(dt)
            pinned = noised(xr, z, sched[j + 1], m1, m2) if fix_mode == "renoise" and j < n - 1 else xr
            y = torch.where(fixed.reshape(-1, 1), pinned, y)
        x = y.reshape(1, L, 4)
        traj.append(x.clone())
        row = (math.nan,) * 4
        if snr[j] != 0:
            s, _ = O.network(sd, b, x, sched[j + 1].to(dt).repeat_interleave(L), static)
            x, row, _ = correct(b, x, s.reshape(1, L, 4), corrector_noise64(L, key, j), snr[j], fixed)
        corr.append(row)
        if eta is not None and eta[j + 1] != 0:
            x = nudge(b, x, eta[j + 1], cap, fixed)[0]
    return x, traj, corr


@functools.lru_cache(maxsize=None)
def reference4(L, dt):
    """The restatement's three-step SDE run of complex L with a corrector behind steps 0 and 1: (init fp32, chi, traj, corr)."""
    b = cpu(L)
    init = initial_state(b, KEYS[L])
    if dt == torch.float64:
        out = corrected_run(sd64(weights_cpu()), cast(b, dt), init.double(), SNR4, mode="sde", key=KEYS[L], sched=SCHED4)
    else:
        out = corrected_run(weights_cpu(), b, init, SNR4, mode="sde", key=KEYS[L], sched=SCHED4)
    return (init,) + out


def self_distance4(L):
    """(the restatement's own fp32 <-> fp64 wrapped distance over the entries that did not flip, the fraction of the movable entries
    that did): over every trajectory step and the final angles.  Flipped: the two precisions are more than 0.1 rad apart."""
    a, b64 = reference4(L, torch.float32), reference4(L, torch.float64)
    mov = movable(cpu(L))
    d = torch.stack([wrapped_absdiff(x.double(), y) for x, y in zip(a[2] + [a[1]], b64[2] + [b64[1]])]).max(0).values
    flipped = (d > 0.1) & mov
    return float(d[~flipped].max()), float(flipped.sum()) / float(mov.sum()), flipped


# ---- schedule.corrector_snr / resolve_corrector -----------------------------------------------------------------------------------------
def test_corrector_snr_values():
    from packppi_amd.schedule import CORRECTOR_DEFAULTS, corrector_snr, resolve_corrector
    assert CORRECTOR_DEFAULTS == dict(snr=0.16, t_on=1.0, last=False)
    f = np.float32
    e = corrector_snr(SCHED)
    assert e.dtype == np.float32 and e.tolist() == [f(0.16)] * 5 + [0]
    assert corrector_snr(SCHED, 0.16, last=True).tolist() == [f(0.16)] * 6
    assert corrector_snr(SCHED, 0.3, t_on=0.5).tolist() == [0, 0, f(0.3), f(0.3), f(0.3), 0]         # schedule[j + 1] <= 0.5 from j = 2
    assert corrector_snr(SCHED, 0.3, t_on=0.0, last=True).tolist() == [0, 0, 0, 0, 0, f(0.3)]
    assert corrector_snr(SCHED, 0.0).tolist() == [0] * 6
    assert corrector_snr(SCHED2, 0.16).tolist() == [0] and corrector_snr(SCHED2, 0.16, last=True).tolist() == [f(0.16)]
    assert resolve_corrector(0.16, SCHED).tolist() == e.tolist()
    assert resolve_corrector(dict(snr=0.3, t_on=0.5), SCHED).tolist() == corrector_snr(SCHED, 0.3, t_on=0.5).tolist()
    assert resolve_corrector(dict(last=True), SCHED).tolist() == [f(0.16)] * 6
    seq = [0.1, 0, 0.2, 0, 0, 0.3]
    for given in (seq, np.float64(seq), torch.tensor(seq), dict(snr=seq)):
        got = resolve_corrector(given, SCHED)
        assert got.dtype == np.float32 and got.tolist() == np.float32(seq).tolist()


def test_corrector_snr_refusals():
    from packppi_amd.schedule import corrector_snr, resolve_corrector
    for bad in (-0.1, math.nan, math.inf):
        with pytest.raises(ValueError, match="finite"):
            corrector_snr(SCHED, bad)
        with pytest.raises(ValueError, match="finite"):
            resolve_corrector([0.1, bad, 0, 0, 0, 0], SCHED)
    with pytest.raises(ValueError, match="t_on"):
        corrector_snr(SCHED, 0.16, t_on=math.nan)
    with pytest.raises(ValueError, match="at least 2"):
        corrector_snr(SCHED[:1])
    with pytest.raises(ValueError, match="entries"):
        resolve_corrector([0.1] * 7, SCHED)                     # one entry per reverse step, not per time
    with pytest.raises(ValueError, match="unknown keys"):
        resolve_corrector(dict(scale=0.1), SCHED)
    with pytest.raises(ValueError, match="bool"):
        resolve_corrector(True, SCHED)


# ---- schedule.step_correct: the reference's function, to the letter -------------------------------------------------------------------
def test_step_correct_is_the_batch_mean():
    """Two complexes of 1 and 2 rows, every number written out.  Masked entries: complex 0 has (0, 0), (0, 1); complex 1 has (1, 0),
    (2, 0), (2, 1), (2, 2).  score norms sqrt(9 + 16) = 5 and sqrt(1 + 4 + 4 + 16) = 5 -> mean 5; noise norms sqrt(1 + 1 + ...):
    complex 0 sqrt(4 + 0) = 2, complex 1 sqrt(1 + 4 + 4 + 16) = 5 -> mean 3.5.  step = 2 (snr 3.5 / 5)^2; with snr = 1: 0.98.
    Per complex it would be 2 (2 / 5)^2 = 0.32 for complex 0 and 2 for complex 1: entry (0, 0) tells them apart."""
    from packppi_amd.schedule import step_correct
    x = torch.tensor([[0.1, 0.2, 0.3, 0.4], [1.0, 1.1, 1.2, 1.3], [2.0, 2.1, 2.2, 2.3]], dtype=torch.float64)
    score = torch.tensor([[3., 4., 7., 7.], [1., 9., 9., 9.], [2., 2., 4., 5.]], dtype=torch.float64)
    noise = torch.tensor([[2., 0., 5., 5.], [1., 8., 8., 8.], [2., 2., 4., 6.]], dtype=torch.float64)
    mask = torch.tensor([[1, 1, 0, 0], [1, 0, 0, 0], [1, 1, 1, 0]], dtype=torch.bool)
    batch = torch.tensor([0, 1, 1]).repeat_interleave(4)
    out = step_correct(x, score, batch, mask, snr=1.0, noise=noise)
    step = 2 * (3.5 / 5) ** 2
    assert step == pytest.approx(0.98)
    amp = math.sqrt(2 * step)
    assert float(out[0, 0]) == pytest.approx(0.1 + 0.98 * 3 + 1.4 * 2, abs=1e-12) and amp == pytest.approx(1.4)
    assert abs(float(out[0, 0]) - (0.1 + 0.32 * 3 + math.sqrt(0.64) * 2)) > 1.0           # not the per-complex step size
    want = x + step * score + amp * noise
    assert torch.allclose(out[mask], want[mask], atol=1e-12, rtol=0)
    assert torch.equal(out[~mask], x[~mask])                                               # masked-out entries keep their bits
    assert torch.equal(x, torch.tensor([[0.1, 0.2, 0.3, 0.4], [1.0, 1.1, 1.2, 1.3], [2.0, 2.1, 2.2, 2.3]], dtype=torch.float64))
    # fp32 input stays fp32, and without explicit noise the call draws (a different result per call)
    a, b = (step_correct(x.float(), score.float(), batch, mask) for _ in range(2))
    assert a.dtype == torch.float32 and not torch.equal(a, b) and torch.equal(a[~mask], x.float()[~mask])
    # the default snr is the reference's
    import inspect
    assert inspect.signature(step_correct).parameters["snr"].default == 0.16


# ---- the argument rules of sampling(corrector=) ---------------------------------------------------------------------------------------
def test_sampling_corrector_argument_rules():
    from packppi_amd.module import TDiffusionModule
    b = complex_cpu(24, 5)
    run = lambda mode, **kw: TDiffusionModule.sampling(_Probe(mode), b, **kw)
    for mode in ("ode", "sde"):
        with pytest.raises(ValueError, match="corrector needs seed"):
            run(mode, corrector=0.16)
    with pytest.raises(ValueError, match="corrector and sde_noise exclude each other"):
        run("sde", corrector=0.16, sde_noise=torch.zeros(6, 2, 24, 4))
    with pytest.raises(ValueError, match="exclude each other"):                   # with a seed today's refusal of the pair comes first
        run("sde", corrector=0.16, seed=1, sde_noise=torch.zeros(6, 2, 24, 4))
    for bad in (-1.0, math.nan, math.inf, [0.1, -0.2, 0, 0, 0, 0]):
        with pytest.raises(ValueError, match="finite"):
            run("ode", corrector=bad, seed=1)
    with pytest.raises(ValueError, match="entries"):
        run("ode", corrector=[0.1, 0.2], seed=1)
    with pytest.raises(ValueError, match="unknown keys"):
        run("ode", corrector=dict(rate=1.0), seed=1)
    with pytest.raises(ValueError, match="fixed_mask needs seed"):                 # the existing refusals come first
        run("ode", corrector=0.16, fixed_mask=torch.zeros(1, 24, dtype=torch.bool))
    with pytest.raises(ValueError, match="guide needs seed in sde mode"):
        run("sde", corrector=0.16, guide=0.02)
    for kw in (dict(), dict(guide=0.02), dict(fixed_mask=torch.zeros(1, 24, dtype=torch.bool)), dict(return_trajectory=True)):
        with pytest.raises(AssertionError, match="reached the device"):           # a valid request goes on to the context
            run("sde", corrector=0.16, seed=1, **kw)
    with pytest.raises(ValueError, match="return_trajectory needs fixed_mask"):   # corrector=None: today's rule, untouched
        run("ode", seed=1, return_trajectory=True)
    import inspect
    for name in ("sampling", "repack", "sample_ensemble", "repack_ensemble", "mutate"):
        assert inspect.signature(getattr(TDiffusionModule, name)).parameters["corrector"].default is None, name


@pytest.mark.parametrize("name", ["eval_diffusion", "mutate"])
def test_command_lines_take_the_flags(name):
    import importlib
    from .test_guided_host import BASE, TODAY
    mod = importlib.import_module(f"packppi_amd.cli.{name}")
    p = mod.build_parser()
    seeded = BASE[name] if "--seed" in BASE[name] else BASE[name] + ["--seed", "1"]
    plain = p.parse_args(BASE[name])
    assert sorted(vars(plain)) == TODAY[name] and mod.corrector_from_args(plain) is None
    a = p.parse_args(seeded + ["--corrector", "0.16"])
    assert mod.corrector_from_args(a, p) == dict(snr=0.16)
    a = p.parse_args(seeded + ["--corrector", "0.2", "--corrector_from", "0.5"])
    assert mod.corrector_from_args(a, p) == dict(snr=0.2, t_on=0.5)
    for bad in (["--corrector_from", "0.5"], ["--corrector", "-1"], ["--corrector", "nan"]):
        with pytest.raises(SystemExit):
            mod.corrector_from_args(p.parse_args(seeded + bad), p)
    if "--seed" not in BASE[name]:
        with pytest.raises(SystemExit):
            mod.corrector_from_args(p.parse_args(BASE[name] + ["--corrector", "0.16"]), p)
    assert "reference's constant" in p.format_help().replace("\n", " ")


def test_corrector_csv(tmp_path):
    from types import SimpleNamespace
    from packppi_amd.cli.eval_diffusion import write_corrector_csv
    nan = math.nan
    trace = torch.tensor([[[1.0, 2.0, 0.5, 1.0], [nan] * 4], [[nan] * 4, [3.0, 4.0, 0.25, 0.75]]], dtype=torch.float64)
    write_corrector_csv(SimpleNamespace(schedule=torch.tensor([1.0, 0.5, 0.0]), corrector_traces=[(None, trace)]), str(tmp_path))
    lines = open(tmp_path / "corrector.csv").read().splitlines()
    assert lines == ["step,t,complex,s2,n2,eps,amp", "0,0.5,0,1.0,2.0,0.5,1.0", "1,0.0,0,,,,", "0,0.5,1,,,,", "1,0.0,1,3.0,4.0,0.25,0.75"]


# ---- the ABI ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    from packppi_amd.build import build_library
    return build_library(verbose=False)


def test_header_and_library_name_the_export(lib_path):
    src = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    decl = re.search(r"pp_status pp_sample_corrected\((.*?)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S), flags=re.S)
    assert decl is not None
    names = [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")]
    assert names == ["ctx", "chi", "chi_ref", "fixed", "fix_mode", "schedule", "n_schedule", "mode", "seed", "snr", "eta", "cap", "chi_traj",
                     "clash_trace", "corr_trace", "stream"]
    assert hasattr(ctypes.CDLL(lib_path), "pp_sample_corrected")
    from packppi_amd import lib
    assert "pp_sample_corrected" in lib.SYMBOLS
    import inspect
    sig = inspect.signature(lib.Context.sample_corrected)
    assert list(sig.parameters)[1:14] == ["chi", "schedule", "mode", "seed", "snr", "eta", "cap", "chi_ref", "fixed", "fix_mode", "trajectory",
                                          "want_trace", "want_corr"]
    assert sig.parameters["eta"].default is None and sig.parameters["cap"].default == 0.1
    from packppi_amd.build import SOURCES
    assert "pp_correct.hip" in SOURCES


# ---- the restatement itself ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,pinned", [("ode", False), ("sde", False), ("sde", True)])
def test_zero_snr_is_the_guided_restatement(mode, pinned):
    """fp64, L = 24: with snr all zero the corrected loop is test_guided_host.guided_run with eta zero, and with an eta it is that
    run with the eta -- bit for bit, every trajectory step."""
    b = cpu(24)
    fx, ref = (fixed_rows(24), rolled(b).double()) if pinned else (None, None)
    init = initial_state(b, KEYS[24], fx, rolled(b) if pinned else None).double()
    sd, b64 = sd64(weights_cpu()), cast(b, torch.float64)
    zero = np.zeros(6, dtype=np.float32)
    for eta in (None, ETA_CONST):
        want = guided_run(sd, b64, init, eta if eta is not None else np.zeros(7, dtype=np.float32), CAP, mode, KEYS[24], fx, ref)
        got = corrected_run(sd, b64, init, zero, eta, CAP, mode, KEYS[24], fx, ref)
        assert torch.equal(got[0], want[0]) and all(torch.equal(a, c) for a, c in zip(got[1], want[1]))
        assert all(math.isnan(v) for row in got[2] for v in row)


def test_restated_corrector_rules():
    """The corrector as the definition states it, on the L = 24 complex at random angles with the oracle's score."""
    b = cpu(24)
    g = torch.Generator().manual_seed(24)
    x = ((torch.rand(b["SC_D"].shape, generator=g) * 2 - 1) * np.pi) * b["SC_D_mask"]
    s, _ = O.network(weights_cpu(), b, x, SCHED[3].repeat_interleave(24))
    s = s.reshape(1, 24, 4)
    z = corrector_noise64(24, KEYS[24], 2)
    y, (s2, n2, eps, amp), mov = correct(b, x, s, z, SNR)
    assert mov.any() and (~mov).any() and torch.equal(y[~mov], x[~mov])
    assert 0.01 < eps < 1 and amp == float(np.float32(math.sqrt(2 * eps)))
    assert eps == pytest.approx(2 * (float(np.float32(SNR)) * math.sqrt(n2) / math.sqrt(s2)) ** 2, rel=1e-6)       # the reference's formula
    assert int((wrapped_absdiff(y, x)[mov] > 0.01).sum()) >= 30 and float(y.abs().max()) <= math.pi + 1e-6
    # the draws are those of counter step 2^20 + j: disjoint from every reverse step's and unlike them
    assert not torch.equal(z, corrector_noise64(24, KEYS[24], 3))
    assert not np.array_equal(words(SEED, (24,), (KEYS[24],), CORR_STEP + 2), words(SEED, (24,), (KEYS[24],), 2))
    # fixed rows are never moved and never counted
    fixed = torch.arange(24) % 2 == 0
    yf, (s2f, _, _, _), movf = correct(b, x, s, z, SNR, fixed)
    assert torch.equal(yf[0, fixed], x[0, fixed]) and not movf[0, fixed].any() and s2f < 0.99 * s2
    # a non-finite score takes its entry out; a segment without a movable entry or with a zero score has no corrector
    k = tuple(torch.nonzero(mov)[0].tolist())
    sn = s.clone()
    sn[k] = math.inf
    yn, rown, movn = correct(b, x, sn, z, SNR)
    assert not movn[k] and yn[k] == x[k] and math.isfinite(rown[0]) and rown[0] < s2
    for args in ((s, torch.ones(24, dtype=torch.bool)), (torch.zeros_like(s), None)):
        y0, row0, _ = correct(b, x, args[0], z, SNR, args[1])
        assert torch.equal(y0, x) and all(math.isnan(v) for v in row0)


@pytest.mark.parametrize("L", [24, 40])
def test_whole_run_cases_are_within_the_flip_cap(L):
    """The three-step SDE run of the GPU test, in the restatement alone: at most 2 % of the movable entries flip (fp32 and fp64 more
    than 0.1 rad apart); every corrector has 0.01 < eps < 1."""
    d, frac, _ = self_distance4(L)
    corr = reference4(L, torch.float32)[3]
    print(f"L = {L}: restatement fp32 <-> fp64 distance off the flipped entries = {d:.3g} rad, flipped fraction = {frac:.4f}; "
          f"eps = {[r[2] for r in corr]}, amp = {[r[3] for r in corr]}")
    assert frac <= 0.02
    assert all(0.01 < r[2] < 1 for r in corr[:2]) and all(math.isnan(v) for v in corr[2])
