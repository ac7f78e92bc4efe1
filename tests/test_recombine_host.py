"""Recombination of decoy ensembles per residue (csrc/pp_recombine.hip): the arithmetic restated in NumPy fp64,
and what can be checked of the entry without a device.

The restatement follows the header comment of pp_ensemble_recombine: the self term U(r, d), the pair term W(r, d; r', d'), the static
partner predicate P (k_clash_cand's), the sweep with its conflict rule, and the trace.  Its objective is checked against
oracle.ref_cpu.residue_clash, which knows nothing of the decomposition.  tests/test_recombine_gpu.py compares the device with it.

Inputs A, B, C: synthetic complexes of 33, 64 and 97 rows with four random decoys each -- the smallest shapes at which the conflict
rule, the cross-decoy indexing and a partner walk over more than one 64-row window (97 rows) can go wrong."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTF, TOL = 12.0, 0.5
CASES = {"A": (33, 4, "uniform"), "B": (64, 4, "uniform"), "C": (97, 4, "near")}
SWEEPS = {"A": 13, "B": 19, "C": 26}                 # sweeps in which a row moves (fp64)


# ---- the restatement (fp64) ------------------------------------------------------------------------------------------------------
def _double(batch):
    from packppi_amd.batch import Batch
    return Batch({k: (v.double() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v) for k, v in batch.items()})


def decoy_angles(batch, n, D, kind):
    """float32 [D, L, 4]: the decoys of complex n, from rng = default_rng(170 + n + 1)."""
    rng = np.random.default_rng(170 + n + 1)
    L = int(batch.max_size)
    m = batch.SC_D_mask[0].double().numpy()
    if kind == "uniform":
        x = rng.uniform(-np.pi, np.pi, (D, L, 4)) * m
    else:
        x = ((batch.SC_D[0].double().numpy() + rng.normal(0, 0.6, (D, L, 4)) + np.pi) % (2 * np.pi) - np.pi) * m
    return torch.from_numpy(x).float()


def partners(batch, tol=TOL):
    """bool [L, L]: P(r), the predicate of k_clash_cand -- another row, another residue_index, |CA - CA'| < e + e' + (3.6 - tol)."""
    from .test_clash_capacity import row_extents
    X = batch.X[0].double().numpy()
    e = row_extents(X, batch.residue_type[0].numpy(), batch.atom_mask[0].numpy())
    ca = X[:, 1]
    dist = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    ri = batch.residue_index[0].numpy()
    return (ri[:, None] != ri[None]) & ~np.eye(len(ri), dtype=bool) & (dist < e[:, None] + e[None] + (3.6 - tol))


def terms(batch, chis, vtf=VTF, tol=TOL):
    """(U [L, D], W [L, D, L, D]) of the header comment in fp64 for the decoys chis [D, L, 4] of the B = 1 host batch."""
    from oracle import ref_cpu as O
    from packppi_amd import constants as rc
    b = _double(batch)
    S, ex = b.residue_type[0], b.atom_mask[0]
    D, L = chis.shape[0], chis.shape[1]
    lo, up = rc.make_atom14_dists_bounds(overlap_tolerance=tol, bond_length_tolerance_factor=vtf)
    lo, up = torch.as_tensor(lo, dtype=torch.float64)[S], torch.as_tensor(up, dtype=torch.float64)[S]
    xyz = torch.stack([O.atom14_coords(b.X, b.residue_type, b.BB_D, chis[d].double()[None])[0] for d in range(D)])   # [D, L, 14, 3]
    nsc = ex[:, 4:].sum(-1)
    inv = (1.0 / (nsc + 1e-10)).numpy()
    U = np.stack([(O.within_residue_violation(xyz[d], ex, lo, up)[:, 4:].sum(-1) / (nsc + 1e-10)).numpy() for d in range(D)], 1)
    # the pair term over the partner pairs only (every other pair is zero at any angles: the comparison with the oracle, which looks
    # at all pairs, would show a missing one): allowed atom pairs [n, 14, 14] and their weights, 8192 row pairs at a time
    exn, ri = ex.numpy() != 0, b.residue_index[0].numpy()
    rad = (ex * torch.as_tensor(rc.between_radius, dtype=torch.float64)[S]).numpy()
    sc = (np.arange(14) >= 4).astype(np.float64)
    bb = np.zeros((14, 14), bool)
    bb[:4, :4] = True
    bb[5, 5] = True
    cn = np.zeros((14, 14), bool)
    cn[2, 0] = True                                                # C of the lower row, N of the higher
    p = xyz.numpy()
    W = np.zeros((L, D, L, D))
    rr, qq = np.nonzero(partners(batch, tol))
    for c0 in range(0, len(rr), 8192):
        r, q = rr[c0:c0 + 8192], qq[c0:c0 + 8192]
        ok = exn[r][:, :, None] & exn[q][:, None, :] & ~bb & (ri[r] != ri[q])[:, None, None]
        ok &= ~((ri[r] + 1 == ri[q])[:, None, None] & cn) & ~((ri[q] + 1 == ri[r])[:, None, None] & cn.T)
        cw = sc[None, :, None] * inv[r][:, None, None] + sc[None, None, :] * inv[q][:, None, None]
        thr = rad[r][:, :, None] + rad[q][:, None, :] - tol
        for d in range(D):
            for e in range(D):
                dist = np.sqrt(1e-10 + ((p[d][r][:, :, None] - p[e][q][:, None, :]) ** 2).sum(-1))
                W[r, d, q, e] = (np.maximum(thr - dist, 0.0) * ok * cw).sum((-2, -1))
    return U, W


def objective(U, W, s):
    """F(s) = sum_r U(r, s_r) + 1/2 sum_r sum_r' W(r, s_r; r', s_r')."""
    r = np.arange(len(s))
    return U[r, s].sum() + 0.5 * W[r, s][:, r, s].sum()


def local_energy(U, W, s):
    """E [L, D]: E_r(d | s) = U(r, d) + sum_r' W(r, d; r', s_r')."""
    return U + W[:, :, np.arange(len(s)), s].sum(-1)


def descend(U, W, P, start, max_sweeps, naive=False):
    """The sweep of the header comment from s = start everywhere: (s, trace of clash(s) = F(s) / L, sweeps in which a row moved,
    converged).  ``naive``: every positive proposal is accepted at once -- the rule the conflict rule replaces."""
    L = U.shape[0]
    s = np.full(L, int(start))
    rows = np.arange(L)
    trace, moved_sweeps, converged = [objective(U, W, s) / L], 0, U.shape[1] == 1
    for _ in range(max_sweeps):
        if converged:
            trace.append(trace[-1])
            continue
        E = local_energy(U, W, s)
        prop = E.argmin(1)                                         # the lowest d wins ties
        gain = np.where(prop == s, 0.0, E[rows, s] - E[rows, prop])
        pos = gain > 0
        if not pos.any():
            converged = True
            trace.append(trace[-1])
            continue
        if naive:
            take = pos
        else:
            beats = (gain[:, None] > gain[None]) | ((gain[:, None] == gain[None]) & (rows[:, None] < rows[None]))
            take = pos & ~(P & pos[None] & ~beats).any(1)
        s = np.where(take, prop, s)
        moved_sweeps += 1
        trace.append(objective(U, W, s) / L)
    return s, np.array(trace), moved_sweeps, converged


class Case:
    """One named input and what the restatement says about it: computed once, shared (the GPU tests import it), never modified."""

    def __init__(self, name):
        from packppi_amd import synth
        from packppi_amd.featurize import protein_to_batch
        n, D, kind = CASES[name]
        self.name, self.n, self.D = name, n, D
        self.b = protein_to_batch(synth.make_complex(n, 170 + n))
        self.chis = decoy_angles(self.b, n, D, kind)

    @functools.cached_property
    def UW(self):
        return terms(self.b, self.chis)

    @functools.cached_property
    def P(self):
        return partners(self.b)

    @functools.cached_property
    def best(self):
        U, W = self.UW
        return int(np.argmin([objective(U, W, np.full(self.n, d)) for d in range(self.D)]))

    @functools.cached_property
    def run(self):
        U, W = self.UW
        return descend(U, W, self.P, self.best, 64)


@functools.lru_cache(maxsize=None)
def case(name):
    return Case(name)


# ---- the restatement against the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_decomposition_is_the_clash_loss(name):
    """F of every decoy and of the recombined structure equals the sum of ref_cpu.residue_clash at those angles to 1e-9 relative.
    The restated W is computed over the pairs of P only and the oracle over all pairs: P holds every pair that contributes."""
    from oracle import ref_cpu as O
    c = case(name)
    U, W = c.UW
    b64 = _double(c.b)
    s, trace, n_sweeps, conv = c.run
    rows = np.arange(c.n)
    structures = [(np.full(c.n, d), c.chis[d]) for d in range(c.D)] + [(s, c.chis[torch.from_numpy(s), torch.arange(c.n)])]
    for sel, chi in structures:
        want = float(O.residue_clash(b64, chi.double()[None], VTF, TOL).sum())
        got = objective(U, W, sel)
        assert abs(got - want) <= 1e-9 * abs(want), (name, got, want)
    assert np.allclose(W, W.transpose(2, 3, 0, 1), rtol=1e-12, atol=0)
    moved = int((s != c.best).sum())
    print(f"{name}: best decoy {c.best}, mean clash {trace[0]:.4f} -> {trace[-1]:.4f}, {n_sweeps} sweeps, {moved} rows moved")


@pytest.mark.parametrize("name", list(CASES))
def test_descent_is_strictly_monotone(name):
    c = case(name)
    s, trace, n_sweeps, conv = c.run
    assert conv and n_sweeps == SWEEPS[name], (name, n_sweeps)
    assert (np.diff(trace[:n_sweeps + 1]) < 0).all() and (trace[n_sweeps:] == trace[n_sweeps]).all()
    # a local optimum: no row can lower F alone
    U, W = c.UW
    E = local_energy(U, W, s)
    assert (E[np.arange(c.n), s] <= E.min(1)).all()
    # accepted rows of one sweep are never partners: replay the first sweep
    s1 = descend(U, W, c.P, c.best, 1)[0]
    acc = s1 != c.best
    assert acc.any() and not c.P[np.ix_(acc, acc)].any()


@pytest.mark.parametrize("name", list(CASES))
def test_accepting_every_proposal_is_not_monotone(name):
    """What the conflict rule is for: with every positive proposal accepted at once the trace rises on these inputs, so the
    monotonicity check of the GPU tests can fail."""
    c = case(name)
    U, W = c.UW
    trace = descend(U, W, c.P, c.best, 64, naive=True)[1]
    rise = np.diff(trace).max()
    print(f"{name}: accept-all raises the mean clash by up to {rise:.2e} in one sweep")
    assert rise > 1e-3, (name, rise)                   # 50 times and more what the GPU test allows a sweep (2e-5)


# ---- the entry, without a device -------------------------------------------------------------------------------------------------
def test_header_binding_and_libraries_agree():
    from packppi_amd import build
    from packppi_amd.lib import SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    diag = re.search(r"#ifdef PP_DIAG\n(.*?)#endif", hdr, flags=re.S)
    assert "pp_ensemble_recombine" in SYMBOLS
    assert re.search(r"pp_status\s+pp_ensemble_recombine\s*\(", hdr.replace(diag.group(0), ""))
    assert "pp_ensemble_recombine" not in diag.group(1)
    assert "pp_recombine.hip" in build.SOURCES and len(build.product_flag_stamps()) == 4
    assert build.embedded_build_id(build.build_library(verbose=False)) == build.build_id(build.FLAGS, build.SOURCES)
    for path in (build.LIB, build.other_variant_path(), build.check_variant_path(), build.diag_variant_path()):
        if os.path.exists(path):
            assert build.embedded_build_id(path).split("-")[1] in build.product_flag_stamps(), path
            assert hasattr(ctypes.CDLL(path), "pp_ensemble_recombine"), path


def test_recombine_refuses_null_arguments_before_the_device():
    from packppi_amd import build
    lib = ctypes.CDLL(build.build_library(verbose=False))
    lib.pp_last_error.restype = ctypes.c_char_p
    vp, i = ctypes.c_void_p, ctypes.c_int
    lib.pp_ensemble_recombine.argtypes = [vp, vp, i, vp, i, vp, vp, vp, vp, vp, vp, vp]
    assert lib.pp_ensemble_recombine(None, None, 2, None, 4, None, None, None, None, None, None, None) == 1
    assert b"pp_ensemble_recombine" in lib.pp_last_error()


def test_cli_refusals(capsys):
    from packppi_amd.cli import eval_diffusion
    base = ["--input", "x.pdb", "--outdir", "out", "--molprobity_clash_loc", "/nonexistent"]
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(base + ["--seed", "1", "--recombine"])
    assert "--recombine needs --n_decoys" in capsys.readouterr().err
    args = eval_diffusion.parse_args(base + ["--n_decoys", "4", "--seed", "1", "--recombine", "--recombine_sweeps", "9"])
    assert args.recombine and args.recombine_sweeps == 9
    args = eval_diffusion.parse_args(base + ["--n_decoys", "4", "--seed", "1"])
    assert not args.recombine and args.recombine_sweeps == 64
