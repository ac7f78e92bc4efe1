"""Obstacle atoms on the device, through the C ABI (pp_ctx_set_obstacles).

References: the UNMODIFIED oracle (chain as obstacles) and the restatement tests/test_obstacles_host.py builds and anchors to it on
the CPU.  Bounds: 5e-5 on per_res (the project's bar); the restatement's own fp32-against-fp64 distance for gradients and angles.
Nothing measured on the device enters a bound."""
import ctypes as C
import functools
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import ref_cpu as O

from . import test_obstacles_host as H
from .conftest import wrapped_absdiff

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTF, TOL, LAMDA = H.VTF, H.TOL, 1.0
CAP = 256                                        # PP_OBSTACLE_CAP of include/packppi_hip.h
FAR = torch.tensor([[900.0, -700.0, 800.0, 1.8], [905.0, -700.0, 800.0, 1.7], [-1000.0, 1000.0, 1000.0, 1.52]])


def new_ctx(batch, obstacles=None, ranges=None):
    """A fresh geometry context of ``batch`` (moved to the device; the context keeps it alive), optionally with obstacles."""
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    gb = batch.to(DEV)
    ctx = Context(geometry_plan(torch.device(DEV)), gb)
    ctx._keep = gb
    if obstacles is not None:
        ctx.set_obstacles(obstacles, ranges)
    return ctx


# ---- 1. chain as obstacles: against the unmodified oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("L,seed", H.ANCHOR_CASES)
def test_chain_as_obstacles_against_the_unmodified_oracle(L, seed):
    full, part, rows_a, chi, obstacles = H.chain_as_obstacles(L, seed)
    want = O.residue_clash(H.cast(full, torch.float64), chi.double(), VTF, TOL)[0, rows_a]
    ob = obstacles(torch.float64)
    ctx = new_ctx(part, ob.float())
    got = ctx.clash(chi[:, rows_a], VTF, TOL)[0].cpu().double()
    active = int((H.residue_clash_obst(H.cast(part, torch.float64), chi[:, rows_a].double(), ob, parts=True) > 0).sum())
    d = (got - want).abs().max().item()
    print(f"chain as obstacles L {L} seed {seed}: {ob.shape[0]} obstacle atoms, {active} rows of A with a term, max |per_res - oracle| {d:.2e}")
    assert active >= 3 and d <= 5e-5
    # without the obstacles chain A alone is another number: the term is what closes the gap
    ctx.set_obstacles(None)
    assert (ctx.clash(chi[:, rows_a], VTF, TOL)[0].cpu().double() - want).abs().max().item() > 1e-2


# ---- 2. value and gradient ------------------------------------------------------------------------------------------------------------
def test_value_and_gradient_against_the_restatement():
    b, chi, ob, rows = H.value_case()
    pr64, g64 = H.clash_and_grad_obst(H.cast(b, torch.float64), chi.double(), ob.double())
    pr32, g32 = H.clash_and_grad_obst(b, chi, ob)
    ctx = new_ctx(b, ob)
    pr, g = ctx.clash(chi, VTF, TOL, need_grad=True)
    pr, g = pr.cpu().double(), g.cpu().double()
    dv = (pr - pr64).abs().max().item()
    env = torch.clamp(4 * (g32.double() - g64).abs(), min=3e-7)
    dg = (g - g64).abs()
    print(f"value and gradient L 33: max |per_res - fp64| {dv:.2e}; max |dchi - fp64| {dg.max().item():.2e}, largest excess over the "
          f"envelope {(dg - env).max().item():.2e}; restatement fp32 vs fp64 {(g32.double() - g64).abs().max().item():.2e}")
    assert dv <= 5e-5
    assert (dg <= env).all()
    # the obstacles push: the gradient differs from the one without them on the rows they touch, and only there the value moves
    ctx.set_obstacles(None)
    pr0, g0 = ctx.clash(chi, VTF, TOL, need_grad=True)
    touched = torch.zeros(33, dtype=torch.bool)
    touched[rows] = True
    share = H.residue_clash_obst(H.cast(b, torch.float64), chi.double(), ob.double(), parts=True)[0]
    assert ((pr[0] - pr0[0].cpu().double()).abs()[share == 0] == 0).all() and (share[touched] > 0).all()
    assert (g[0, touched] - g0[0, touched].cpu().double()).abs().max() > 1e-4
    # exact zeros on rows without a chi angle
    none = b.SC_D_mask[0].sum(-1) == 0
    assert none.any() and (g[0, none] == 0).all()


# ---- 3. nothing leaks ------------------------------------------------------------------------------------------------------------------
def test_far_obstacles_and_a_cleared_set_change_no_bit():
    b, chi, ob, _ = H.proximal_case()
    fresh = new_ctx(b)
    pr0, g0 = fresh.clash(chi, VTF, TOL, need_grad=True)
    run0 = fresh.proximal_packed(chi, VTF, TOL, LAMDA, 8, want_traj=True)
    far = new_ctx(b, FAR)
    pr1, g1 = far.clash(chi, VTF, TOL, need_grad=True)
    assert torch.equal(pr1, pr0) and torch.equal(g1, g0)
    for x, y in zip(far.proximal_packed(chi, VTF, TOL, LAMDA, 8, want_traj=True), run0):
        assert torch.equal(x, y)
    ctx = new_ctx(b, ob)
    pr2 = ctx.clash(chi, VTF, TOL)
    assert not torch.equal(pr2, pr0)
    assert not torch.equal(ctx.proximal_packed(chi, VTF, TOL, LAMDA, 8)[1], run0[1])
    ctx.set_obstacles(None)
    assert ctx.n_obstacles == 0
    pr3, g3 = ctx.clash(chi, VTF, TOL, need_grad=True)
    assert torch.equal(pr3, pr0) and torch.equal(g3, g0)
    for x, y in zip(ctx.proximal_packed(chi, VTF, TOL, LAMDA, 8, want_traj=True), run0):
        assert torch.equal(x, y)
    # and back again, with a smaller set in the kept allocation
    ctx.set_obstacles(ob[:5])
    ctx.set_obstacles(ob)
    assert torch.equal(ctx.clash(chi, VTF, TOL), pr2)


def test_refusals_and_the_sticky_flag():
    from packppi_amd import lib as L
    from packppi_amd import synth
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_data
    b, chi, ob, _ = H.proximal_case()
    ctx = new_ctx(b)
    l, s = L.load(), L._stream(torch.device(DEV))
    x = ob.to(DEV).contiguous()
    whole = np.ascontiguousarray([[0, 12]], dtype=np.int32)                   # kept alive: the calls read this host table
    rng = C.c_void_p(whole.ctypes.data)
    assert l.pp_ctx_set_obstacles(None, L._ptr(x), rng, 12, s) == 1
    for first, count in ((0, 13), (-1, 5), (10, 3), (0, -1)):
        keep = np.ascontiguousarray([[first, count]], dtype=np.int32)
        assert l.pp_ctx_set_obstacles(ctx.handle, L._ptr(x), C.c_void_p(keep.ctypes.data), 12, s) == 1, (first, count)
        assert b"range" in l.pp_last_error()
    assert l.pp_ctx_set_obstacles(ctx.handle, L._ptr(x), None, 12, s) == 1 and l.pp_ctx_set_obstacles(ctx.handle, L._ptr(x), rng, -1, s) == 1
    with pytest.raises(ValueError):
        ctx.set_obstacles(ob, [(0, 13)])
    with pytest.raises(ValueError):
        ctx.set_obstacles(torch.tensor([[0.0, 0.0, float("nan"), 1.7]]))
    # nothing of that installed a set
    assert torch.equal(ctx.clash(chi, VTF, TOL), new_ctx(b).clash(chi, VTF, TOL)) and ctx.saturated() == 0
    # a padded B > 1 context
    pad = new_ctx(collate([protein_to_data(synth.make_complex(40, 2)), protein_to_data(synth.make_complex(36, 3))]))
    keep = np.ascontiguousarray([[0, 12], [0, 12]], dtype=np.int32)
    assert l.pp_ctx_set_obstacles(pad.handle, L._ptr(x), C.c_void_p(keep.ctypes.data), 12, s) == 1 and b"padded" in l.pp_last_error()
    # a bad value in a DEVICE tensor is found on the device: bit 2 of the sticky word
    for bad in (torch.tensor([[0.0, float("inf"), 0.0, 1.7]]), torch.tensor([[0.0, 0.0, 0.0, -1.0]])):
        c2 = new_ctx(b)
        assert c2.saturated() == 0
        c2.set_obstacles(bad.to(DEV))
        assert c2.saturated() == 4


# ---- 4. packing invariance -------------------------------------------------------------------------------------------------------------
def test_a_complex_gets_the_bits_of_running_alone():
    from packppi_amd import synth
    from packppi_amd.batch import pack
    from packppi_amd.featurize import protein_to_batch
    b, chi_a, ob, _ = H.proximal_case()                                     # 64 rows, with obstacles
    a = H.Batch(b)
    a["obstacle_xyzr"], a["obstacle_offsets"], a["obstacle_offsets_host"] = ob, torch.tensor([0, 12], dtype=torch.int32), [0, 12]
    other = protein_to_batch(synth.make_complex(40, 7))                     # without
    g = torch.Generator().manual_seed(5)
    chi_o = ((torch.rand(1, 40, 4, generator=g) * 2 - 1) * np.pi) * other.SC_D_mask
    for order in ((a, other), (other, a)):
        pk = pack(order)
        assert pk.obstacle_offsets_host == ([0, 12, 12] if order[0] is a else [0, 0, 12])
        chi = torch.cat([chi_a if c is a else chi_o for c in order], 1)
        fixed = torch.zeros(1, 104, dtype=torch.bool)
        fixed[0, ::3] = True
        ctx = new_ctx(pk)
        assert ctx.n_obstacles == 12
        lo = 0
        for c in order:
            n = c.X.shape[1]
            solo = new_ctx(c)
            x = chi[:, lo:lo + n]
            assert torch.equal(ctx.clash(chi, VTF, TOL)[:, lo:lo + n], solo.clash(x, VTF, TOL))
            for fx in (None, fixed):
                kw = {} if fx is None else dict(fixed=fx, return_moved=True)
                skw = {} if fx is None else dict(fixed=fx[:, lo:lo + n], return_moved=True)
                p = ctx.proximal_packed(chi, VTF, TOL, LAMDA, 6, want_traj=True, **kw)
                q = solo.proximal_packed(x, VTF, TOL, LAMDA, 6, want_traj=True, **skw)
                seg = 0 if c is order[0] else 1
                assert torch.equal(p[0][:, :, lo:lo + n], q[0]) and torch.equal(p[1][:, lo:lo + n], q[1])
                assert torch.equal(p[2][:, lo:lo + n], q[2]) and torch.equal(p[3][seg], q[3][0])
                if fx is not None:
                    assert torch.equal(p[4][:, lo:lo + n], q[4])
            lo += n


# ---- 5. proximal -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _prox_refs():
    b, chi, ob, rows = H.proximal_case()
    r32 = H.proximal_obst(b, chi, ob, num_steps=10)
    r64 = H.proximal_obst(H.cast(b, torch.float64), chi.double(), ob.double(), num_steps=10)
    return r32, r64


def test_proximal_against_the_restatement():
    b, chi, ob, rows = H.proximal_case()
    (c32, l32, m32), (c64, l64, m64) = _prox_refs()
    ctx = new_ctx(b, ob)
    traj, last, acc, losses, moved = ctx.proximal_packed(chi, VTF, TOL, LAMDA, 50, want_traj=True,
                                                         fixed=torch.zeros(1, 64, dtype=torch.bool), return_moved=True)
    assert torch.equal(moved.cpu(), m64) and moved[0, rows.to(DEV)].all()          # the rows overlapping obstacles are in the mask
    ls = losses[0].cpu().double().numpy()
    rel = np.abs(ls[:10] / np.array(l32) - 1).max()
    firm = m64[..., None].expand(-1, -1, 4) & b.SC_D_mask.bool()
    div = np.array([float(wrapped_absdiff(x, y)[firm].max()) for x, y in zip(c32, c64)])
    d = np.array([float(wrapped_absdiff(traj[t].cpu(), c32[t])[firm].max()) for t in range(10)])
    env = np.maximum(2e-5, 8 * div)
    print(f"proximal with obstacles: loss rel vs fp32 restatement {rel:.2e}; angles vs fp32 " + " ".join(f"{v:.1e}" for v in d)
          + "; restatement fp32 vs fp64 " + " ".join(f"{v:.1e}" for v in div) + f"; loss {ls[0]:.5f} -> {ls[-1]:.5f}")
    assert np.allclose(ls[:10], np.array(l32), rtol=5e-5, atol=0), rel
    assert (d <= env).all(), (d.tolist(), env.tolist())
    still = ~m64[0]
    assert all(torch.equal(traj[t].cpu()[0, still], chi[0, still]) for t in range(50))
    # the loss goes down and the obstacle share of the overlapped rows with it
    assert ls[-1] < ls[0] and torch.equal(acc, last)
    share = lambda x: H.residue_clash_obst(H.cast(b, torch.float64), x.cpu().double(), ob.double(), parts=True)[0, rows].sum().item()
    assert share(last) < share(chi)
    # bit-reproducible, on the same context and on a fresh one; pp_proximal is the same loop
    again = ctx.proximal_packed(chi, VTF, TOL, LAMDA, 50, want_traj=True)
    other = new_ctx(b, ob).proximal(chi, VTF, TOL, LAMDA, 50, want_traj=True)
    assert torch.equal(again[0], traj) and torch.equal(again[3], losses)
    assert torch.equal(other[0], traj) and torch.equal(other[2], losses[0])


# ---- 6. capacity -----------------------------------------------------------------------------------------------------------------------
def capacity_case(n_near, seed=6):
    """(batch of 33 rows with a lysine at row K, chi, obstacles [n_near + 40, 4]): n_near obstacle atoms inside the reach of the
    lysine's row (|CA - q| < e + r_o + 1.8 - tol), 40 far outside everybody's; no atom within 0.05 A of any row's limit."""
    from packppi_amd import constants as rc
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    from .test_clash_capacity import _protein, row_extents
    p = synth.make_complex(33, 21)
    K = 16
    aatype = p["aaindex"].copy()
    aatype[K] = rc.restype_order["K"]
    g = np.random.default_rng(seed)
    chi = g.uniform(-np.pi, np.pi, (33, 4))
    b = protein_to_batch(_protein(p["atom_positions"][:, :4], aatype, chi, p))
    X = b.X[0].double().numpy()
    e = row_extents(X, b.residue_type[0].numpy(), b.atom_mask[0].numpy())
    ca = X[:, 1]
    pts = []
    while len(pts) < n_near:
        ro = float(g.choice([1.7, 1.55, 1.52, 1.8]))
        u = g.normal(size=3)
        q = ca[K] + u / np.linalg.norm(u) * (e[K] + ro + 1.8 - TOL) * g.uniform(0.0, 1.0) ** (1 / 3) * 0.97
        if (np.abs(np.linalg.norm(ca - q, axis=1) - (e + ro + 1.8 - TOL)) > 0.05).all():
            pts.append(np.r_[q, ro])
    far = np.c_[ca[K] + 200.0 + g.uniform(0, 30, (40, 3)), np.full(40, 1.7)]
    ob = torch.from_numpy(np.float32(np.r_[np.array(pts), far][g.permutation(n_near + 40)]))
    return b, b.SC_D.clone(), ob, K


def restated_counts(b, ob):
    """[L] obstacles o with r_o > 0 and |CA_i - q_o| < e_i + r_o + 1.8 - tol (fp64), -1 above the capacity."""
    from .test_clash_capacity import row_extents
    X = b.X[0].double().numpy()
    e = row_extents(X, b.residue_type[0].numpy(), b.atom_mask[0].numpy())
    q = ob.double().numpy()
    dist = np.linalg.norm(X[:, 1][:, None] - q[None, :, :3], axis=-1)
    n = ((dist < e[:, None] + q[None, :, 3] + 1.8 - TOL) & (q[None, :, 3] > 0)).sum(1)
    return np.where(n <= CAP, n, -1)


CAPACITY_AMOUNTS = (CAP - 37, CAP, 3 * CAP)


def _hashes():
    """Child process (diagnostic library, PP_CLASH_SCAN = 0 or 1): sha256 of the proximal runs of test 5 and of the three capacity
    cases, and the per-row static obstacle counts pp_debug_buffer(9) reads back."""
    from packppi_amd import lib as L
    out = {}
    b, chi, ob, _ = H.proximal_case()
    cases = [("prox", b, chi, ob)] + [(f"cap{n}",) + capacity_case(n)[:3] for n in CAPACITY_AMOUNTS]
    for name, b, chi, ob in cases:
        ctx = new_ctx(b, ob)
        traj, last, acc, losses = ctx.proximal_packed(chi, VTF, TOL, LAMDA, 12, want_traj=True)
        raw = torch.zeros(b.X.shape[1], dtype=torch.float32, device=DEV)
        l = L.load()
        l.pp_debug_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
        assert l.pp_debug_buffer(ctx.handle, 9, C.c_void_p(raw.data_ptr()), raw.numel()) == 0, l.pp_last_error()
        out[name] = dict(hash=hashlib.sha256(traj.cpu().numpy().tobytes() + losses.cpu().numpy().tobytes()).hexdigest(),
                         counts=raw.view(torch.int32).cpu().tolist(),
                         last=hashlib.sha256(last.cpu().numpy().tobytes()).hexdigest())
    print("RESULT " + json.dumps(out))


@functools.lru_cache(maxsize=None)
def _child_runs():
    from packppi_amd.build import diag_variant_path
    assert os.path.exists(diag_variant_path()), "libpackppi_hip.dbg.so not built (__graft_entry__.build() builds it)"
    code = "import sys; sys.path.insert(0, %r)\nfrom tests import test_obstacles_gpu as T\nT._hashes()\n" % ROOT
    outs = []
    for scan in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PP_CLASH_SCAN=scan, PACKPPI_LIB=diag_variant_path()),
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][0][7:]))
    return outs


def test_candidate_path_and_scan_path_agree_bit_for_bit():
    cand, scan = _child_runs()
    assert set(cand) == {"prox"} | {f"cap{n}" for n in CAPACITY_AMOUNTS}
    for name in cand:
        assert cand[name]["hash"] == scan[name]["hash"] and cand[name]["last"] == scan[name]["last"], name
    # and the product library gives those bits too
    b, chi, ob, _ = H.proximal_case()
    traj, last, acc, losses = new_ctx(b, ob).proximal_packed(chi, VTF, TOL, LAMDA, 12, want_traj=True)
    assert hashlib.sha256(traj.cpu().numpy().tobytes() + losses.cpu().numpy().tobytes()).hexdigest() == cand["prox"]["hash"]


@pytest.mark.parametrize("n_near", CAPACITY_AMOUNTS)
def test_capacity_of_the_static_obstacle_lists(n_near):
    """A lysine with n_near obstacle atoms in reach: below, exactly at and three times beyond the per-row capacity (256).  The counts
    the device kept equal the numpy restatement of the reach rule, row for row (-1 = the row scans); per_res equals the fp64
    restatement within 5e-5 x max(1, |per_res|) -- the project's bar for values of order one, carried as a relative bound where
    hundreds of hinges add up to a larger number -- and the gradient stays inside the restatement's own fp32 / fp64 envelope; the
    candidate run and the scan run agree bit for bit (test above)."""
    b, chi, ob, K = capacity_case(n_near)
    want = restated_counts(b, ob)
    assert want[K] == (n_near if n_near <= CAP else -1)
    cand, scan = _child_runs()
    got = np.array(cand[f"cap{n_near}"]["counts"])
    print(f"capacity {n_near}: restated count of the lysine row {want[K]}, device {got[K]}; rows that scan {int((want < 0).sum())}, "
          f"largest list {want.max()}")
    assert (got == want).all(), (got.tolist(), want.tolist())
    pr64, g64 = H.clash_and_grad_obst(H.cast(b, torch.float64), chi.double(), ob.double())
    pr32, g32 = H.clash_and_grad_obst(b, chi, ob)
    pr, g = new_ctx(b, ob).clash(chi, VTF, TOL, need_grad=True)
    pr, g = pr.cpu().double(), g.cpu().double()
    tol = 5e-5 * torch.clamp(pr64.abs(), min=1.0)
    env = torch.clamp(4 * (g32.double() - g64).abs(), min=3e-7)
    print(f"  per_res of the lysine {pr64[0, K].item():.4f}; max |per_res - fp64| {(pr - pr64).abs().max().item():.2e}; "
          f"max |dchi - fp64| {(g - g64).abs().max().item():.2e}")
    assert ((pr - pr64).abs() <= tol).all() and pr64[0, K] > 1.0
    assert ((g - g64).abs() <= env).all()


# ---- 7. recombination --------------------------------------------------------------------------------------------------------------------
def test_recombination_counts_the_obstacles():
    from packppi_amd.batch import replicate
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd import synth
    D, n = 4, 40
    p = synth.make_complex(n, 7)
    plain = protein_to_batch(p)
    g = torch.Generator().manual_seed(77)
    chis = ((torch.rand(D, n, 4, generator=g) * 2 - 1) * np.pi) * plain.SC_D_mask
    ob, rows = H.place_near_terminals(plain, chis[0:1], 6, 3, 0.4, 1.2, seed=40, overlap=True)
    b = protein_to_batch(p, obstacles=dict(xyz=ob[:, :3].numpy(), radius=ob[:, 3].numpy()))
    pb = replicate(b.to(DEV), D)
    assert pb.obstacle_offsets_host == [0, 18] and len(pb.seg_offsets_host) == D + 1
    ctx = new_ctx(pb)
    assert ctx.n_obstacles == 18
    chi = chis.reshape(1, D * n, 4).to(DEV).contiguous()
    per_res = ctx.clash(chi, VTF, TOL)
    red = ctx.ensemble_reduce(chi, D, per_res=per_res, select="clash")
    rec = ctx.ensemble_recombine(chi, D, start=red.best, max_sweeps=64, vtf=VTF, tol=TOL)
    trace = rec.clash_trace[0].cpu().numpy()
    start = int(red.best[0])
    one = new_ctx(replicate(b.to(DEV), 1))
    first = float(one.clash(chi[:, start * n:(start + 1) * n], VTF, TOL).double().mean())
    final = float(one.clash(rec.chi, VTF, TOL).double().mean())
    one.set_obstacles(None)
    bare = float(one.clash(rec.chi, VTF, TOL).double().mean())
    print(f"recombine with obstacles: trace {trace[0]:.6f} -> {trace[-1]:.6f} in {int(rec.sweeps[0])} sweeps; Context.clash at the start "
          f"{first:.6f}, at the recombined angles {final:.6f} (without the obstacles {bare:.6f})")
    assert abs(trace[0] - first) <= 5e-5 and abs(trace[0] - float(red.clash[start])) <= 5e-5
    assert abs(trace[-1] - final) <= 5e-5
    assert final - bare > 1e-3                                    # the identity holds because the term is in U, not without it
    assert (np.diff(trace) <= 2e-5).all() and trace[-1] < trace[0]
    # a group whose decoys point at different ranges is left alone
    ctx.set_obstacles(ob, [(0, 18), (0, 18), (0, 17), (0, 18)])
    bad = ctx.ensemble_recombine(chi, D, start=red.best, max_sweeps=4, vtf=VTF, tol=TOL)
    assert bool((bad.pick == -1).all()) and bool(torch.isnan(bad.clash_trace).all()) and int(bad.sweeps[0]) == 0
    ctx.set_obstacles(ob, [(0, 18)] * D)
    again = ctx.ensemble_recombine(chi, D, start=red.best, max_sweeps=64, vtf=VTF, tol=TOL)
    assert torch.equal(again.pick, rec.pick) and torch.equal(again.clash_trace, rec.clash_trace)


# ---- 8. command line ---------------------------------------------------------------------------------------------------------------------
def test_eval_diffusion_with_and_without_the_flag(tmp_path):
    import gzip
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.pdb_io import from_pdb_file, obstacle_atoms
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd import batch as B
    src = str(tmp_path / "T1124_lig.pdb")
    with gzip.open(H.LIG, "rt") as fh, open(src, "w") as out:
        out.write(fh.read())
    base = ["--input", src, "--molprobity_clash_loc", "none", "--use_proximal", "--random_weights", "0", "--seed", "7", "--steps", "5",
            "--device", DEV]
    outs = {}
    for name, extra in (("with", ["--obstacles", "hetero"]), ("without", []), ("none", ["--obstacles", "none"])):
        d = tmp_path / name
        eval_diffusion.main(base + ["--outdir", str(d)] + extra)
        outs[name] = d
    text = (outs["with"] / "structure.pdb").read_text().split("\n")
    het = [ln.rstrip("\n") for ln in open(src) if ln.startswith("HETATM")]
    assert len(het) == 132
    at = max(i for i, ln in enumerate(text) if ln.startswith("TER")) + 1
    assert text[at:at + 132] == het and text[at + 132].startswith("ENDMDL")
    # without the flag (or with none): no HETATM, no csv, byte-equal outputs
    plain = (outs["without"] / "structure.pdb").read_bytes()
    assert b"HETATM" not in plain and plain == (outs["none"] / "structure.pdb").read_bytes()
    assert sorted(os.listdir(outs["without"])) == sorted(os.listdir(outs["none"])) and not (outs["without"] / "obstacles.csv").exists()
    # obstacles.csv against two Context.clash calls, at the input's angles and at the written structure's
    rows = [ln.split(",") for ln in (outs["with"] / "obstacles.csv").read_text().strip().split("\n")]
    assert rows[0] == ["residue", "chain", "clash_obstacles_before", "clash_obstacles_after"]
    protein = from_pdb_file(src)
    assert [int(r[0]) for r in rows[1:]] == [int(x) for x in protein["residue_index"]] and [r[1] for r in rows[1:]] == list(protein["chain_id"])
    b = protein_to_batch(protein, obstacles=obstacle_atoms(src)).to(DEV)
    bare = new_ctx(B.Batch({k: v for k, v in b.items() if k not in B.OBSTACLE_KEYS}))
    ctx = new_ctx(b)
    share = lambda chi: (ctx.clash(chi, 12.0, 0.5) - bare.clash(chi, 12.0, 0.5))[0].cpu().numpy()
    before = np.array([float(r[2]) for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(before, share(b.SC_D))
    # the seeded run again, in process: the same angles, so the same column
    args = eval_diffusion.parse_args(base + ["--outdir", str(tmp_path / "again"), "--obstacles", "hetero"])
    chi = eval_diffusion.load_model(args).sampling(b, use_proximal=True, seed=7)
    after = np.array([float(r[3]) for r in rows[1:]], dtype=np.float32)
    assert np.array_equal(after, share(chi))
    print(f"eval_diffusion --obstacles hetero: clash against the 78 obstacle atoms, summed over residues, {before.sum():.4f} at the "
          f"input's angles, {after.sum():.4f} at the result's; {(after > 0).sum()} residues touch them")
