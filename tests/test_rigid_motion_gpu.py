"""GPU: every geometry kernel on structures far from the origin and in arbitrary orientation.

Inputs, motions, references and the conditions the references satisfy on their own: tests/test_rigid_motion_host.py.  Every device
result is compared with the fp64 oracle (or a test module's restatement) on the SAME featurised batch, never with the unmoved
structure's result.  Bars: for a quantity with an existing bar beta the moved-input bar is max(beta, 3 d_ref), d_ref = |oracle fp32 -
oracle fp64| on the same batch, pooled as the maximum over the rotations of that shift length (the factor 3 of the envelope tests of
tests/test_hip_parity.py); the ``id`` motion is held to beta alone.  Clash and its gradient: max(2.5e-6 max |per_res|, 4 d_ref) and
max(3e-7, 4 d_ref) of test_clash_capacity.test_scan_path_against_fp64, residues at a hinge threshold left out.  Nothing measured on
the device enters a bar.

PACKPPI_RIGID_REPORT=<file> appends every measured distance next to its d_ref and bar (profiles/r25_rigid_motion.txt).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from . import test_rigid_motion_host as H
from .conftest import wrapped_absdiff

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTF, TOL, LAMDA = H.VTF, H.TOL, H.LAMDA
FAR = "R1@3000"


def _report(line):
    print(line)
    path = os.environ.get("PACKPPI_RIGID_REPORT")
    if path:
        libname = os.path.basename(os.environ.get("PACKPPI_LIB") or "libpackppi_hip.so")
        with open(path, "a") as fh:
            fh.write(f"{libname:24s} {line}\n")


def _check(cid, what, d, d_ref, bar):
    _report(f"{cid:10s} {what:34s} device {d:.2e}  d_ref {d_ref:.2e}  bar {bar:.2e}")
    assert d <= bar, (cid, what, d, d_ref, bar)


@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    return TDiffusionModule(weights, device=DEV)


def _geometry_ctx(batch):
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    ctx = Context(geometry_plan(torch.device(DEV)), batch)
    ctx._keep = batch
    return ctx


# ---- 1. graph ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.GRAPH_CASES)
def test_neighbour_sets_and_edge_embedding(cid, model):
    """The fp64 oracle's neighbour sets row by row; h_E0 by neighbour against the fp64 oracle on the edges j != i and against the fp32
    oracle on the edges j == i (arccos of coplanar normals: rounding noise of up to pi that the kernel reproduces, tests/test_hip_parity
    test_graph).

    The control of the j != i comparison is NOT held to beta = 2e-5 against fp64: that beta is test_graph's bar against the reference's
    fp32 tensor, and the reference's own fp32 arithmetic misses it against fp64 on input A at the origin -- measured on the CPU, |oracle
    fp32 - oracle fp64| = 6.02e-5 there, all of it the pair dihedral phi of edge (26, 16), which lies 2.1e-4 rad from -pi where the
    unclamped arccos turns one ulp of its argument into 2.1e-4 rad (device against fp64: 6.01e-5).  So ``id`` gets max(beta, 3 d_ref)
    against fp64 like every other motion, and beta where beta belongs: against the fp32 oracle, on every real edge."""
    c = H.case(cid)
    E, hE = model._context(c.device_batch(DEV)).graph()
    bar, d_ref = H.bar(cid, H.BETA["hE0"], lambda k: max(g["d_ref"] for g in H.graph_ref(k)), control_at_beta=False)
    worst, worst_self, worst_32 = 0.0, 0.0, 0.0
    for b, g, E_s, h_s in zip(c.parts, H.graph_ref(cid), c.cut(E), c.cut(hE)):
        valid = g["valid"]
        idx, h = H._sorted_edges(E_s, h_s)
        assert torch.equal(idx[0][valid], g["idx"][0][valid])                 # the fp64 oracle's neighbour sets, row by row
        use = g["real"] & ~g["self_edge"]
        worst = max(worst, float((h.double() - g["hE64"])[use].abs().max()))
        own = g["real"] & g["self_edge"]
        worst_self = max(worst_self, float((h - g["hE32"])[own].abs().max()))
        worst_32 = max(worst_32, float((h - g["hE32"])[use].abs().max()))
    _check(cid, "hE0 j != i vs fp64", worst, d_ref, bar)
    if cid.endswith("-id"):
        _check(cid, "hE0 j != i vs fp32 oracle", worst_32, 0.0, H.BETA["hE0"])
    else:
        _report(f"{cid:10s} {'hE0 j != i vs fp32 oracle':34s} device {worst_32:.2e}  (no bar)")
    _check(cid, "hE0 j == i vs fp32 oracle", worst_self, 0.0, H.BETA["hE0"])


# ---- 2. an exact translation changes no list -------------------------------------------------------------------------------------------
def test_exact_translation_changes_no_neighbour_list(weights):
    """Coordinates on a 2^-9 A grid (and a 3.75 A lattice full of equal distances) shifted by (2048, -3072, 2560): every coordinate and
    every CA difference is exact in float32 before and after, so a search that works from differences returns the same lists entry
    for entry, ties included; one that forms |a|^2 + |b|^2 - 2 a.b, or splits absolute coordinates, does not."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.module import TDiffusionModule
    from .test_hip_parity import _tie_batch
    snapped = synth.snap_to_grid(H.protein_of("A"))
    a0, a1 = protein_to_batch(snapped), protein_to_batch(synth.rigid_motion(snapped, None, H.EXACT_SHIFT))
    t0 = _tie_batch(300, 307, 3.75)
    t1 = t0.clone()
    t1["X"] = t0.X + torch.tensor(H.EXACT_SHIFT)
    for b0, b1 in ((a0, a1), (t0, t1)):
        ca0, ca1 = b0.X[0, :, 1].double(), b1.X[0, :, 1].double()
        assert torch.equal(ca1, ca0 + torch.tensor(H.EXACT_SHIFT, dtype=torch.float64))
        assert torch.equal(b0.X[0, :, 1][:, None] - b0.X[0, :, 1][None], b1.X[0, :, 1][:, None] - b1.X[0, :, 1][None])
    ca = t1.X[:, :, 1, :]
    S = ((ca[:, None] - ca[:, :, None]) ** 2).sum(3) + 1e-6
    D_exact = torch.from_numpy(np.sqrt(S.numpy()))
    E_ref = torch.topk(D_exact, 32, dim=-1, largest=False)[1]
    ranked = torch.sort(D_exact[0], -1)[0]
    assert int((ranked[:, 31] == ranked[:, 32]).sum()) > 50                   # membership ties at rank K on many rows
    for mode in ("aten_cpu", "lower_index", "aten_member"):
        m = TDiffusionModule(weights, device=DEV, knn_ties=mode)
        for name, b0, b1 in (("snapped A", a0, a1), ("lattice 300", t0, t1)):
            E0 = m._context(b0.to(DEV)).graph()[0].cpu()
            E1 = m._context(b1.to(DEV)).graph()[0].cpu()
            differ = int((E0 != E1).sum())
            _report(f"exact translation, {name}, {mode}: list entries that differ {differ}")
            assert differ == 0, (name, mode)
            if name == "lattice 300" and mode == "aten_cpu":
                assert torch.equal(E1, E_ref)


# ---- 3. network ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.NETWORK_CASES)
def test_network_at_three_times(cid, model):
    c = H.case(cid)
    gb = c.device_batch(DEV)
    chi = c.join(c.chi).to(DEV)
    refs = H.network_ref(cid)
    for what in ("score", "hV"):
        bar, d_ref = H.bar(cid, H.BETA[what], lambda k: H.network_dref(k, what))
        for tval, tn in H.TIMES:
            t = torch.tensor([tval]).repeat_interleave(c.n_rows)
            out = model.network(gb, chi, t)[0 if what == "score" else 1]
            d = max(float((o.double() - r[64][f"{what}_{tn}"])[b.residue_mask.bool()].abs().max())
                    for b, r, o in zip(c.parts, refs, c.cut(out)))
            _check(cid, f"{what} {tn} vs fp64", d, d_ref, bar)
    assert model._context(gb).saturated() == 0


@pytest.mark.parametrize("cid", H.NETWORK_CASES)
def test_ten_ode_steps(cid, model):
    c = H.case(cid)
    ctx = model._context(c.device_batch(DEV))
    out = ctx.sample(c.join(c.chi).to(DEV), torch.linspace(1, 0, 11))
    bar, d_ref = H.bar(cid, H.BETA["sampling"], lambda k: H.network_dref(k, "sampling"))
    d = 0.0
    for b, r, o in zip(c.parts, H.network_ref(cid), c.cut(out)):
        m = b.SC_D_mask.bool()
        d = max(d, float(wrapped_absdiff(o, r[64]["ode"])[m].max()))
        assert (o[~m] == 0).all()
    _check(cid, "ten ODE steps vs fp64 (rad)", d, d_ref, bar)
    assert ctx.saturated() == 0


# ---- 4. atom14, clash, gradient --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.GEOMETRY_CASES)
def test_atom14_clash_and_gradient(cid):
    c = H.case(cid)
    gb = c.device_batch(DEV)
    ctx = _geometry_ctx(gb)
    chi = c.join(c.chi).to(DEV)
    xyz = ctx.atom14(chi)
    pr, grad = ctx.clash(chi, VTF, TOL, need_grad=True)
    refs = H.geometry_ref(cid)
    bar_x, dref_x = H.bar(cid, H.BETA["atom14"], lambda k: H.geometry_dref(k, "atom14"))
    dref_pr = max(H.geometry_dref(k, "clash") for k in H.pool(cid))
    dref_g = max(H.geometry_dref(k, "grad") for k in H.pool(cid))
    bar_pr = max(2.5e-6 * max(float(r["pr64"].abs().max()) for r in refs), 4 * dref_pr)
    bar_g = max(3e-7, 4 * dref_g)
    dx = dp = dg = 0.0
    for b, r, x, p, g in zip(c.parts, refs, c.cut(xyz), c.cut(pr), c.cut(grad)):
        valid = b.residue_mask.bool()
        assert torch.isfinite(x).all() and torch.equal(x[..., :4, :], b.X[..., :4, :])           # the backbone: X bit for bit
        dx = max(dx, float((x.double() - r["xyz64"])[valid].abs().max()))
        dp = max(dp, float((p.double() - r["pr64"]).abs().max()))
        # pp_clash weighs the gradient by 1 / rows of the whole context, the oracle on one part by 1 / rows of the part
        g64 = r["g64"] * (b.residue_type.shape[1] / c.n_rows)
        use = ~r["marginal"]
        dg = max(dg, float((g.double() - g64)[0][use].abs().max()))
        assert not bool(((g64 == 0) & (g != 0))[0][use].any())                                   # exact zeros stay exact zeros
    _check(cid, "atom14 vs fp64 (A)", dx, dref_x, bar_x)
    _check(cid, "per-residue clash vs fp64", dp, dref_pr, bar_pr)
    _check(cid, "clash gradient vs fp64", dg, dref_g, bar_g)


# ---- 5. five proximal steps ------------------------------------------------------------------------------------------------------------
def _proximal(cid):
    c = H.case(cid)
    ctx = _geometry_ctx(c.device_batch(DEV))
    return ctx.proximal(c.chi[0].to(DEV), VTF, TOL, LAMDA, 5)


@pytest.mark.parametrize("cid", H.PROXIMAL_CASES)
def test_five_proximal_steps(cid):
    traj, last, losses = _proximal(cid)
    losses = losses.cpu().double().numpy()
    l32, l64 = H.proximal_ref(cid)
    bar, d_ref = H.bar(cid, H.BETA["loss_rel"], H.proximal_dref)
    assert torch.equal(last, traj[-1]) and np.isfinite(losses).all()
    d = float(np.max(np.abs(losses - l64) / np.maximum(np.abs(l64), 1e-7 / bar)))                # relative, with the 1e-7 floor of allclose
    _check(cid, "five proximal losses vs fp64 (rel)", d, d_ref, bar)


def _print_hashes():
    """Child process (diagnostic library, PP_CLASH_SCAN = 0 or 1): sha256 of five proximal steps of C at R1@3000 and of twelve steps
    of chain A of input A at R1@3000 with chain B as obstacles."""
    traj, last, losses = _proximal(f"C-{FAR}")
    print("hash proximal", hashlib.sha256(traj.cpu().numpy().tobytes() + last.cpu().numpy().tobytes() + losses.cpu().numpy().tobytes()).hexdigest())
    part, chi, ob = H.obstacle_case(FAR)
    ctx = _geometry_ctx(part.to(DEV))
    ctx.set_obstacles(ob)
    traj, last, acc, losses = ctx.proximal_packed(chi.to(DEV), VTF, TOL, LAMDA, 12, want_traj=True)
    print("hash obstacles", hashlib.sha256(traj.cpu().numpy().tobytes() + last.cpu().numpy().tobytes() + losses.cpu().numpy().tobytes()).hexdigest())


def test_candidate_lists_are_a_shortcut_to_the_same_bits_far_from_the_origin():
    """PP_CLASH_SCAN=1 (diagnostic library) makes every wave scan: the static candidate lists -- the protein's and the obstacles' --,
    culled by bounding spheres around coordinates of 3000 A, must lead to the same bits.  C carries zeroed slots 3000 A from its atoms."""
    from packppi_amd.build import diag_variant_path
    assert os.path.exists(diag_variant_path()), "libpackppi_hip.dbg.so not built (__graft_entry__.build() builds it)"
    code = "import sys; sys.path.insert(0, %r)\nfrom tests import test_rigid_motion_gpu as T\nT._print_hashes()\n" % ROOT
    outs = []
    for scan in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PP_CLASH_SCAN=scan, PACKPPI_LIB=diag_variant_path()),
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("hash ")])
    assert len(outs[0]) == 2 and outs[0] == outs[1], outs


# ---- 6. obstacles ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", H.MOTIONS)
def test_obstacles_value_and_gradient(motion):
    r = H.obstacle_ref(motion)
    ctx = _geometry_ctx(r["part"].to(DEV))
    ctx.set_obstacles(r["ob"])
    pr, g = ctx.clash(r["chi"].to(DEV), VTF, TOL, need_grad=True)
    pr, g = pr.cpu().double(), g.cpu().double()
    same = [m for m in H.MOTIONS if H.parse(m)[1] == H.parse(motion)[1] and (m == "id") == (motion == "id")]
    dref_pr, dref_g = max(H.obstacle_dref(m, "clash") for m in same), max(H.obstacle_dref(m, "grad") for m in same)
    use = ~r["marginal"]
    assert int(use.sum()) >= 0.95 * len(use)
    cid = f"A+ob-{motion}"
    _check(cid, "per-residue clash vs fp64", float((pr - r["pr64"]).abs().max()), dref_pr,
           max(2.5e-6 * float(r["pr64"].abs().max()), 4 * dref_pr))
    _check(cid, "clash gradient vs fp64", float((g - r["g64"])[0][use].abs().max()), dref_g, max(3e-7, 4 * dref_g))
    assert not bool(((r["g64"] == 0) & (g != 0))[0][use].any())
    # the obstacles do push: without them the value is another one
    ctx.set_obstacles(None)
    assert float((ctx.clash(r["chi"].to(DEV), VTF, TOL).cpu().double() - r["pr64"]).abs().max()) > 1e-2


# ---- 7. SASA ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.SASA_CASES)
def test_sasa_counts_and_areas(cid):
    from . import test_sasa_host as S
    c32, c64, amb, radius = H.sasa_ref(cid)
    res = _geometry_ctx(H.case(cid).device_batch(DEV)).sasa(want_counts=True, n_points=H.N_POINTS, probe=H.PROBE)
    got = res.counts.reshape(-1, 14, 4).cpu().numpy()
    clear = ~amb.any(-1)
    _report(f"{cid:10s} sasa: words that differ from the fp32 restatement {int((got != c32).sum())}, from fp64 outside ambiguous points "
            f"{int((got[clear] != c64[clear]).sum())} (threshold {H.sasa_threshold(cid):.2e} A^2, ambiguous {amb[radius > 0].mean():.2e})")
    assert got.dtype == np.int32 and got.tobytes() == c32.tobytes()
    assert np.array_equal(got[clear], c64[clear])
    want = S.area_fp64(got, radius, H.PROBE, H.N_POINTS)
    area = res.area.reshape(-1, 4).cpu().double().numpy()
    rel = float(np.max(np.abs(area - want) / np.maximum(np.abs(want), 1e-30)))
    _check(cid, "sasa area vs fp64 sum (rel)", rel, 0.0, 2e-6)
    assert (got[radius <= 0] == 0).all() and float(want[:, 1].sum() - want[:, 2].sum()) > 50.0 and got[..., 2].sum() > 0


# ---- 8. shell --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", H.case_ids("A", ("P",)))
def test_shell_both_modes(cid):
    """The matrix of tests/test_shell_gpu.py (both modes, three radii, four seed sets, the chain flag; the batch's X and atom14 built on
    the device) against the float32 restatement on the same bits, row for row; and, on the batch's X, against the float64 form on every
    row decided by more than 4 ulp32(max |X|) of radius."""
    from .test_shell_gpu import RADII, _run_matrix, _seed_sets
    c = H.case(cid)
    gb = c.device_batch(DEV)
    offs = [0] + [int(v) for v in np.cumsum(c.lens)]
    n = offs[-1]
    a, b = (offs[1], offs[2]) if cid == "P" else (0, n)                       # P: seeds in the far middle segment
    sets = _seed_sets(a, b, n)
    if cid == "P":
        sets["every row"] = np.ones(n, np.uint8)
    assert _run_matrix(gb, offs, sets) == 2 * 2 * 3 * len(sets) * 2
    ctx = _geometry_ctx(gb)
    X, amask = gb.X[0].cpu().numpy(), gb.atom_mask[0].cpu().numpy()
    eps = 4 * H.ulp32(c.max_abs)
    seeds = sets["one"]
    for mode in ("ca", "atom"):
        for radius in RADII:
            got = ctx.shell(torch.from_numpy(seeds).reshape(1, n), radius=radius, mode=mode)[0].cpu().numpy().astype(np.uint8)
            want, decided = H.shell_fp64(X, seeds, offs, radius, mode, amask, eps)
            assert decided.mean() >= 0.9 and np.array_equal(got[decided], want[decided]), (mode, radius)


# ---- 9. recombination energies, ensemble reduce ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("motion", H.MOTIONS)
def test_recombination_energies_and_ensemble_reduce(motion):
    from . import test_recombine_gpu as R
    from . import test_recombine_host as RH
    from .test_ensemble_gpu import MEAN_TOL, _host, _wrapped, consensus64, scores64
    from oracle import ref_cpu as O
    host = H.decoy_case(motion)
    d = R.Dev(host)
    cid = f"A-{motion}"
    same = [m for m in H.MOTIONS if H.parse(m)[1] == H.parse(motion)[1] and (m == "id") == (motion == "id")]
    d_ref = max(H.decoy_case(m).d_ref for m in same)
    # local energies at the start assignment: the existing bar 1e-4 + 4e-6 |E|, or 4 d_ref (the clash's factor: summation order)
    U, W = host.UW
    want = RH.local_energy(U, W, np.full(d.n, d.start))
    err = np.abs(d.rec.energy.cpu().double().numpy() - want)
    extra = 0.0 if motion == "id" else 4 * d_ref
    _report(f"{cid:10s} {'local energies vs fp64':34s} device {err.max():.2e}  d_ref {d_ref:.2e}  bar {max(1e-4, extra):.2e} + 4e-6 |E|")
    assert d.start == host.best and (err <= np.maximum(R.tol_e(want), extra)).all()
    R.check_is_a_recombination(d)
    # the reduction: consensus against fp64, deviation from the stored mean, and the clash score against the fp64 ORACLE's per_res
    mask, m1pi, offs = _host(d.pb)
    x = d.chi[0].cpu().numpy()
    valid = (mask != 0)[:d.n]
    mean_ref, res_ref = consensus64(x, mask, m1pi, offs, d.D)
    mean, res = d.red.mean[0].cpu().numpy(), d.red.resultant[0].cpu().numpy()
    cmp = valid & (res_ref >= 1e-6)
    P = np.where(m1pi[:d.n], np.pi, 2.0 * np.pi)
    assert _wrapped(mean.astype(np.float64) - mean_ref, P)[cmp].max() <= MEAN_TOL
    assert np.abs(res.astype(np.float64) - res_ref)[valid].max() <= 1e-6
    b64 = H.cast(host.b, torch.float64)
    pr64 = np.concatenate([O.residue_clash(b64, xx[None].double(), VTF, TOL)[0].numpy() for xx in host.chis])
    dev_ref, clash_ref = scores64(x, mean, mask, m1pi, pr64, offs, d.D)
    assert np.all(np.abs(d.red.dev.cpu().numpy() - dev_ref) <= 1e-9 * np.abs(dev_ref) + 1e-12)
    dc = float(np.abs(d.red.clash.cpu().numpy() - clash_ref).max())
    _check(cid, "decoy clash scores vs fp64 oracle", dc, d_ref, max(2.5e-6 * float(pr64.max()), extra))
    assert int(d.red.best[0]) == int(np.argmin(clash_ref))


# ---- 10. the exact-fp32 library ----------------------------------------------------------------------------------------------------------
def test_exact_fp32_library():
    """Checks 3 - 5 once more on libpackppi_hip.f32.so, in a fresh child."""
    from packppi_amd.build import other_variant_path
    lib = other_variant_path()
    if os.environ.get("PACKPPI_LIB"):
        pytest.skip("already a child run")
    assert os.path.exists(lib), f"{os.path.basename(lib)} not built (__graft_entry__.build() builds it)"
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                        "-k", "test_network_at_three_times or test_ten_ode_steps or test_atom14_clash_and_gradient or test_five_proximal_steps"],
                       env=dict(os.environ, PACKPPI_LIB=lib), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    n = 2 * len(H.NETWORK_CASES) + len(H.GEOMETRY_CASES) + len(H.PROXIMAL_CASES)
    assert f"{n} passed" in r.stdout
