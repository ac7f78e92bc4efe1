"""The clash kernels' two bounded partner lists at and beyond their capacity ("Round 5: static candidates").

k_clash reaches a residue's partners through the static candidate list of the proximal loop (PP_CL_CAP = 96 entries per (residue,
wave), compacted 64 lanes at a time; a fuller wave keeps the per-step scan, count -1) and through the per-step scan list (CL_MAXC =
2048 entries per wave; a fuller one is drained and the scan resumed).  Real proteins have about a dozen candidates per residue, so
the inputs here are built to leave that regime:

``dense_complex()``: 448 rows, 307 of them rigidly translated into one ball so that every pair of them is a candidate.  Which rows
go into the ball sets the per-(row, wave) counts -- wave w owns the partner windows 64 w + 256 m:
    wave 0 (rows 0..63, 256..319): 97 ball rows -> 96 for a ball row in those windows (itself excluded), 97 for every other ball row
    wave 1 (64..127, 320..383):    80 ball rows -> 79 / 80, the second 64-lane compaction chunk
    wave 2 (128..191, 384..447):  120 ball rows -> 119 / 120, over the capacity: -1, the wave scans
    wave 3 (192..255):             10 ball rows -> 9 / 10
The other 141 rows are the rest of the synthetic complex, dilated about its centroid until no two of them and none of them and the
ball can ever touch (count 0).  (Three waves need two windows each, hence 448 rows and not fewer.)

``collapsed_cloud()``: 8320 copies of residues inside one small ball -- what a collapsed or duplicated structure looks like.  Every
row keeps all 8319 partners, 2080 per wave: more than the 1985 a wave can list before it has to drain and resume.

The references are oracle.ref_cpu in float64 and plain numpy restatements of the culling rules; nothing measured on the device
enters a bound.  Measured distances are recorded in profiles/r16_clash_capacity.txt.
"""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from .conftest import wrapped_absdiff

DEV = "cuda:0"
gpu = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VTF, TOL, LAMDA = 12.0, 0.5, 1.0
CAP, WAVES, MAXC = 96, 4, 2048                  # PP_CL_CAP, CL_WAVES, CL_MAXC of csrc/pp_clash.hip
REACH = 3.6 - TOL                               # largest r_a + r_b - tol (two sulphurs)
DENSE_L = 448
BALL_ROWS = np.r_[0:64, 256:289, 64:128, 320:336, 128:192, 384:440, 192:202]
BALL_TYPES = "RQEHKMFWY"                        # side-chain extent >= 5.2 A: every pair limit in the ball is >= 13.5 A
CLOUD_L = 8320


# ---- numpy restatements (fp64) ---------------------------------------------------------------------------------------------------
def type_extents():
    """[21] the culling bound of pp_api.hip side_chain_extents: max over side-chain atoms of |lit| + sum of |t_k| along the atom's
    rigid-group chain, times 1.0001, plus 1e-3."""
    from packppi_amd import constants as rc
    df = rc.default_frames.astype(np.float64)
    tlen = np.linalg.norm(df[:, :, :3, 3], axis=-1)                                  # [21, 8]
    ext = np.zeros(21)
    for S in range(21):
        m = 0.0
        for a in range(4, 14):
            if rc.atom14_mask[S, a] == 0:
                continue
            g = int(rc.atom14_to_group[S, a])
            b = np.linalg.norm(rc.lit_positions[S, a].astype(np.float64))
            b += tlen[S, 4:g + 1].sum() if g >= 4 else tlen[S, g]
            m = max(m, b)
        ext[S] = m * 1.0001 + 1e-3
    return ext


def row_extents(X, rtype, amask):
    """[L] e of k_clash_cand: the type's bound or the actual distance of N / C / O from CA (x 1.0001 + 1e-3), whichever is larger."""
    X = np.asarray(X, np.float64)
    e = type_extents()[np.asarray(rtype)]
    for a in (0, 2, 3):
        d = np.linalg.norm(X[:, a] - X[:, 1], axis=-1) * 1.0001 + 1e-3
        e = np.where(np.asarray(amask)[:, a] != 0, np.maximum(e, d), e)
    return e


def pair_tables(batch):
    """(CA distance [L, L], pair limit e_i + e_j + 3.6 - tol [L, L], allowed [L, L]: not the row itself, another residue_index)."""
    X = batch.X[0].double().numpy()
    e = row_extents(X, batch.residue_type[0].numpy(), batch.atom_mask[0].numpy())
    ca = X[:, 1]
    dist = np.linalg.norm(ca[:, None] - ca[None], axis=-1)
    ri = batch.residue_index[0].numpy()
    allowed = (ri[:, None] != ri[None]) & ~np.eye(len(ri), dtype=bool)
    return dist, e[:, None] + e[None] + REACH, allowed


def candidate_counts(batch):
    """[L, 4] partners of row i in wave w's windows (64 w + 256 m) that pass |CA_i - CA_j| < e_i + e_j + 3.6 - tol."""
    dist, lim, allowed = pair_tables(batch)
    keep = allowed & (dist < lim)
    wave = (np.arange(keep.shape[0]) // 64) % WAVES
    return np.stack([keep[:, wave == w].sum(1) for w in range(WAVES)], 1)


# ---- inputs ----------------------------------------------------------------------------------------------------------------------
def _points_in_ball(n, radius, min_sep, rng):
    pts = np.zeros((0, 3))
    while len(pts) < n:
        p = rng.uniform(-radius, radius, 3)
        if np.linalg.norm(p) <= radius and (len(pts) == 0 or np.linalg.norm(pts - p, axis=1).min() >= min_sep):
            pts = np.vstack([pts, p])
    return pts


def _protein(bb, aatype, chi, like):
    """Protein dict (synth.make_complex's layout) from backbone [L, 4, 3], types and angles; chains and numbering of `like`."""
    from packppi_amd import constants as rc
    from packppi_amd import synth
    chi = chi * rc.chi_angles_mask[aatype]
    xyz = synth.build_atom14(bb, aatype, chi)
    mask = rc.atom14_mask[aatype].astype(np.float64)
    xyz = np.where(mask[..., None] > 0, xyz, np.nan).astype(np.float32).astype(np.float64)
    return dict(atom_positions=xyz, atom_mask=mask, aaindex=aatype.astype(np.int64), residue_index=like["residue_index"],
                chain_id=like["chain_id"], b_factors=np.zeros((len(aatype), 14)))


def dense_complex(seed=1600):
    """B = 1 batch of DENSE_L rows (module docstring).  Every residue is a rigid body: N, CA, C, O of synth.make_complex translated
    together, the side chain rebuilt from the frames."""
    from packppi_amd import constants as rc
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    p = synth.make_complex(DENSE_L, seed)
    rng = np.random.default_rng(seed + 1)
    bb = p["atom_positions"][:, :4].copy()
    aatype = p["aaindex"].copy()
    ball = np.zeros(DENSE_L, bool)
    ball[BALL_ROWS] = True
    aatype[ball] = rng.choice([rc.restype_order[c] for c in BALL_TYPES], int(ball.sum()))
    ext = type_extents()
    # the ball: any two CAs in it are at most 0.88 x the smallest pair limit apart (the backbone atoms are closer to CA than that bound)
    radius = 0.44 * (2 * ext[aatype[ball]].min() + REACH)
    ca = bb[:, 1].copy()
    ca[ball] = _points_in_ball(int(ball.sum()), radius, 0.3, rng)
    # the rest: dilated about its centroid until any two rows are 1.6 x the largest possible limit apart, then moved as a whole so
    # that the origin (the ball) is that far plus the ball's radius from every one of them
    gap = 1.6 * (2 * max(ext.max(), 2.5) + REACH)
    rest = ca[~ball] - ca[~ball].mean(0)
    dmin = min(np.linalg.norm(np.delete(rest, k, 0) - rest[k], axis=1).min() for k in range(len(rest)))
    rest = rest * (gap / dmin)
    best = None
    for u in rng.normal(size=(500, 3)):
        u /= np.linalg.norm(u)
        for r in np.linspace(0.0, np.linalg.norm(rest, axis=1).max() + gap + radius, 60):
            if np.linalg.norm(rest - r * u, axis=1).min() >= gap + radius:
                if best is None or r < best[0]:
                    best = (r, u)
                break
    ca[~ball] = rest - best[0] * best[1]
    bb = bb + (ca - bb[:, 1])[:, None]
    chi = rng.uniform(-np.pi, np.pi, (DENSE_L, 4))
    return protein_to_batch(_protein(bb, aatype, chi, p))


def collapsed_cloud(seed=1700):
    """(B = 1 batch of CLOUD_L rows, chi [1, L, 4]): copies of one backbone residue, every CA inside a ball of radius 1 A, each row
    with its own type and angles."""
    from packppi_amd import constants as rc
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    p = synth.make_complex(8, seed, n_chains=1)
    rng = np.random.default_rng(seed + 1)
    bb = np.repeat(p["atom_positions"][3:4, :4], CLOUD_L, 0)
    aatype = rng.choice([rc.restype_order[c] for c in BALL_TYPES], CLOUD_L)
    u = rng.normal(size=(CLOUD_L, 3))
    ca = u / np.linalg.norm(u, axis=1, keepdims=True) * (rng.random((CLOUD_L, 1)) ** (1 / 3))
    bb = bb + (ca - bb[:, 1])[:, None]
    like = dict(residue_index=np.arange(1, CLOUD_L + 1, dtype=np.int64), chain_id=np.array(["A"] * CLOUD_L))
    chi = rng.uniform(-np.pi, np.pi, (CLOUD_L, 4))
    b = protein_to_batch(_protein(bb, aatype, chi, like))
    return b, (torch.from_numpy(chi).float() * b.SC_D_mask[0]).unsqueeze(0)


def start_angles(batch, seed=5):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(1, int(batch.max_size), 4, generator=g) * 2 - 1) * 3.0) * batch.SC_D_mask


def _double(batch):
    from packppi_amd.batch import Batch
    return Batch({k: (v.double() if isinstance(v, torch.Tensor) and v.dtype == torch.float32 else v) for k, v in batch.items()})


def marginal_hinge_rows(batch64, chi64, window=1e-5):
    """bool [L]: residues owning an atom pair whose between-residue hinge is within `window` of its threshold (fp64)."""
    from oracle import ref_cpu as O
    from packppi_amd import constants as rc
    S, ex = batch64.residue_type[0], batch64.atom_mask[0]
    xyz = O.atom14_coords(batch64.X, batch64.residue_type, batch64.BB_D, chi64)[0]
    r = ex * torch.as_tensor(rc.between_radius, dtype=torch.float64)[S]
    ri = batch64.residue_index[0]
    hit = torch.zeros(len(S), dtype=torch.bool)
    for i0 in range(0, len(S), 64):                               # [64, L, 14, 14] at a time
        sl = slice(i0, i0 + 64)
        d = torch.sqrt(1e-10 + ((xyz[sl, None, :, None] - xyz[None, :, None, :]) ** 2).sum(-1))
        m = (ex[sl, None, :, None] * ex[None, :, None, :]) != 0
        m &= (ri[sl, None] != ri[None])[..., None, None]
        bbm = torch.zeros(14, 14, dtype=torch.bool)
        bbm[:4, :4] = True
        m &= ~bbm
        near = m & ((r[sl, None, :, None] + r[None, :, None, :] - TOL - d).abs() < window)
        hit[sl] |= near.any(-1).any(-1).any(-1)
        hit |= near.any(-1).any(-1).any(0)
    return hit


# ---- shared state ----------------------------------------------------------------------------------------------------------------
class _Dense:
    """dense_complex(), its start angles and what the oracle says about them: each piece computed once, when a test first asks for it
    (20 to 30 s of CPU time over the whole module, most of it the two 3-step reference optimisations), and never modified."""

    def __init__(self):
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        self.b = dense_complex()
        self.chi = start_angles(self.b)
        self.b64 = _double(self.b)
        self.ball = np.zeros(DENSE_L, bool)
        self.ball[BALL_ROWS] = True

    @functools.cached_property
    def counts(self):
        return candidate_counts(self.b)

    @functools.cached_property
    def grad32(self):
        from oracle import ref_cpu as O
        return O.clash_and_grad(self.b, self.chi, VTF, TOL)

    @functools.cached_property
    def grad64(self):
        from oracle import ref_cpu as O
        return O.clash_and_grad(self.b64, self.chi.double(), VTF, TOL)

    pr32, g32 = property(lambda s: s.grad32[0]), property(lambda s: s.grad32[1])
    pr64, g64 = property(lambda s: s.grad64[0]), property(lambda s: s.grad64[1])

    @functools.cached_property
    def marginal(self):
        return marginal_hinge_rows(self.b64, self.chi.double())

    @functools.cached_property
    def ref32(self):
        from oracle import ref_cpu as O
        return O.proximal_optimizer(self.b, self.chi, VTF, TOL, LAMDA, 3)

    @functools.cached_property
    def ref64(self):
        from oracle import ref_cpu as O
        return O.proximal_optimizer(self.b64, self.chi.double(), VTF, TOL, LAMDA, 3)

    # the oracle's clash mask (ref_cpu.clash_mask: rows above the mean) from the per-residue values already at hand
    mask32 = property(lambda s: (s.pr32 > s.pr32.mean())[..., None].expand(-1, -1, 4))
    mask64 = property(lambda s: (s.pr64 > s.pr64.mean())[..., None].expand(-1, -1, 4))
    # |fp64 gradient| of the first proximal step: the anchor term is 0 at x = z, so lamda x d(mean clash)/dchi on the masked rows
    g0 = property(lambda s: (LAMDA * s.g64 * s.mask64).abs())


@pytest.fixture(scope="module")
def dense():
    return _Dense()


@pytest.fixture(scope="module")
def dense_ctx(dense):
    from packppi_amd.functional import _ctx_for
    gb = dense.b.to(DEV)
    return gb, _ctx_for(gb)


def _diag():
    from packppi_amd import lib as L
    l = L.load()
    if not hasattr(l, "pp_debug_buffer"):
        pytest.skip("needs libpackppi_hip.dbg.so (run through test_diag_library_runs_the_capacity_tests)")
    l.pp_debug_buffer.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    return l


def _timed(t0, name):
    print(f"wall {name}: {time.time() - t0:.2f} s")


# ---- a. host: the culling bound is sound -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def side_chain_maxima():
    """[20] fp64 max |side-chain atom - CA| over 4000 chi vectors per type: uniform in [-pi, pi]^4 plus the 3^4 grid of {-pi, 0, pi/2}."""
    from packppi_amd import synth
    rng = np.random.default_rng(16)
    grid = np.stack(np.meshgrid(*[[-np.pi, 0.0, np.pi / 2]] * 4, indexing="ij"), -1).reshape(-1, 4)
    chi = np.concatenate([rng.uniform(-np.pi, np.pi, (4000 - len(grid), 4)), grid])
    bb1 = synth.make_complex(8, 3, n_chains=1)["atom_positions"][3, :4]
    bb = np.repeat(bb1[None], len(chi), 0)
    from packppi_amd import constants as rc
    out = np.zeros(20)
    for S in range(20):
        aat = np.full(len(chi), S)
        xyz = synth.build_atom14(bb.copy(), aat, chi)
        m = rc.atom14_mask[S, 4:] != 0
        if m.any():
            out[S] = np.linalg.norm(xyz[:, 4:][:, m] - bb1[1], axis=-1).max()
    return out


def test_side_chain_extent_bounds_every_conformation(side_chain_maxima):
    """DESIGN calls plan->side_extent "a rigorous bound": no side-chain atom of any type gets farther from its CA than the restated
    extent at any of 4000 chi vectors (no assertion on how loose it is)."""
    from packppi_amd import constants as rc
    ext = type_extents()
    print("type  max |atom - CA|  extent  slack")
    for S in range(20):
        print(f"{rc.restypes[S]}     {side_chain_maxima[S]:8.4f}      {ext[S]:7.4f}  "
              + (f"{ext[S] / side_chain_maxima[S] - 1:6.1%}" if side_chain_maxima[S] > 0 else "     -"))
        assert side_chain_maxima[S] <= ext[S], (rc.restypes[S], side_chain_maxima[S], ext[S])


# ---- the inputs are what they claim to be (host) --------------------------------------------------------------------------------
def test_dense_complex_spans_the_three_regimes(dense):
    """The conditions on dense_complex(), on the CPU: counts in every regime, a row with static and scanning waves, every sphere test
    decided by a wide margin, and the oracle-only conditions of the gradient and optimiser comparisons."""
    n = dense.counts
    print("candidate counts per (row, wave): " + ", ".join(f"{v}: {c}" for v, c in zip(*np.unique(n, return_counts=True))))
    assert (n <= 64).any() and ((n >= 65) & (n <= 95)).any() and (n == CAP).any() and (n == CAP + 1).any() and (n >= 115).any()
    assert (n[dense.ball, 0] >= CAP).all() and set(n[dense.ball, 1]) == {79, 80} and set(n[dense.ball, 2]) == {119, 120}
    assert ((n > CAP).any(1) & (n <= CAP).any(1)).any()
    assert (n[~dense.ball] == 0).all()
    dist, lim, allowed = pair_tables(dense.b)
    assert (((dist < 0.9 * lim) | (dist > 1.5 * lim))[allowed]).all()
    ca = dense.b.X[0, :, 1].double().numpy()
    assert np.linalg.norm(ca[:, None] - ca[None], axis=-1)[~np.eye(DENSE_L, dtype=bool)].min() >= 0.29
    from packppi_amd import constants as rc
    assert not np.isin(dense.b.residue_type[0].numpy()[dense.ball], [rc.restype_order["G"], rc.restype_order["A"]]).any()
    # (c): hinges at their threshold own at most 2 % of the chi entries
    assert dense.marginal.float().mean() <= 0.02, float(dense.marginal.float().mean())
    # (f): masks agree, the compared entries are well conditioned, few moved entries are left out
    assert torch.equal(dense.mask32, dense.mask64)
    moved = dense.mask64 & dense.b.SC_D_mask.bool()
    firm = moved & (dense.g0 >= 1e-5)
    assert firm.sum() >= 0.9 * moved.sum(), (int(firm.sum()), int(moved.sum()))
    for a, c in zip(dense.ref32[0], dense.ref64[0]):
        assert float(wrapped_absdiff(a, c)[firm].max()) <= 1e-4


@pytest.fixture(scope="module")
def cloud():
    b, chi = collapsed_cloud()
    return b, chi


def test_collapsed_cloud_overflows_one_wave_list(cloud):
    """Every pair of the cloud passes the static rule and, at the test's angles, the per-step centroid-sphere test, both inside 0.9 x
    the limit (fp64): a wave keeps 2080 (2079 where the row itself is in its windows) partners, more than the 1985 after which the scan
    stops for a drain."""
    from packppi_amd import synth
    b, chi = cloud
    assert CLOUD_L < 16384 and len(set(b.residue_index[0].tolist())) == CLOUD_L
    X = b.X[0].double().numpy()
    e = row_extents(X, b.residue_type[0].numpy(), b.atom_mask[0].numpy())
    ca = X[:, 1]
    xyz = synth.build_atom14(X[:, :4].copy(), b.residue_type[0].numpy(), chi[0].double().numpy())
    ex = b.atom_mask[0].numpy() != 0
    cen = (xyz * ex[..., None]).sum(1) / ex.sum(1, keepdims=True)
    rad = (np.linalg.norm(xyz - cen[:, None], axis=-1) * ex).max(1)
    worst = [0.0, 0.0]
    for k, (pt, r) in enumerate(((ca, e), (cen, rad))):              # L x L pairs, 1040 rows at a time
        sq = (pt ** 2).sum(1)
        for i0 in range(0, CLOUD_L, 1040):
            sl = slice(i0, i0 + 1040)
            d2 = np.maximum(sq[sl, None] + sq[None] - 2 * pt[sl] @ pt.T, 0.0)
            worst[k] = max(worst[k], float(np.sqrt((d2 / (r[sl, None] + r[None] + REACH) ** 2).max())))
    print(f"collapsed cloud: largest distance / limit, static rule {worst[0]:.3f}, centroid spheres {worst[1]:.3f}")
    assert worst[0] < 0.9 and worst[1] < 0.9, worst
    per_wave = np.bincount((np.arange(CLOUD_L) // 64) % WAVES)
    assert (per_wave - 1 > MAXC - 64).all(), per_wave


# ---- b. the device tables match the restatement (dbg library) ---------------------------------------------------------------------
@gpu
def test_device_extents_and_candidate_counts(dense, dense_ctx, side_chain_maxima):
    """pp_debug_buffer(8): the plan's side_extent is at least the fp64 maxima of every type and within 1e-5 of the restatement;
    pp_debug_buffer(7) after one proximal call: cand_cnt equals the restated counts entry for entry, -1 above 96 -- the proof that the
    second compaction chunk, the fallback and both sides of the 96 / 97 boundary ran on the device."""
    l = _diag()
    t0 = time.time()
    gb, ctx = dense_ctx
    ext_dev = torch.empty(21, device=DEV)
    assert l.pp_debug_buffer(ctx.handle, 8, C.c_void_p(ext_dev.data_ptr()), 21) == 0, l.pp_last_error()
    ext_dev = ext_dev.cpu().double().numpy()
    assert (ext_dev[:20] >= side_chain_maxima).all()
    assert np.abs(ext_dev - type_extents()).max() <= 1e-5, np.abs(ext_dev - type_extents()).max()
    ctx.proximal(dense.chi.to(DEV), VTF, TOL, LAMDA, 1)
    raw = torch.empty(DENSE_L * WAVES, device=DEV)
    assert l.pp_debug_buffer(ctx.handle, 7, C.c_void_p(raw.data_ptr()), raw.numel()) == 0, l.pp_last_error()
    got = raw.view(torch.int32).cpu().numpy().reshape(DENSE_L, WAVES)
    want = np.where(dense.counts > CAP, -1, dense.counts)
    print("device cand_cnt histogram: " + ", ".join(f"{v}: {c}" for v, c in zip(*np.unique(got, return_counts=True))))
    assert (got == want).all(), np.argwhere(got != want)[:8]
    assert (got == -1).any() and (got == CAP).any() and ((got > 64) & (got < CAP)).any() and ((got >= 0) & (got <= 64)).any()
    _timed(t0, "b device tables")


# ---- c. the scan path on the dense input against fp64 -----------------------------------------------------------------------------
@gpu
def test_scan_path_against_fp64(dense, dense_ctx):
    """pp_clash (every wave scans) on the dense input: per_res and dchi within max(project bar, 4 x |oracle fp32 - oracle fp64|) of the
    fp64 oracle -- the bars of test_clash_gradient_at_reference_iterates, 2.5e-6 x max |per_res| and 3e-7; the factor 4 is for the
    kernel's summation order (4 stripes x 4 waves, then the within-residue terms) against torch's.  The gradient jumps where a hinge
    sits at its threshold: the chi of residues owning such an atom pair (fp64, within 1e-5 A) are left out, at most 2 % of all."""
    t0 = time.time()
    gb, ctx = dense_ctx
    pr, dchi = ctx.clash(dense.chi.to(DEV), VTF, TOL, need_grad=True)
    pr, dchi = pr.cpu().double()[0], dchi.cpu().double()[0]
    use = ~dense.marginal
    pr32, pr64, g32, g64 = dense.pr32[0].double(), dense.pr64[0], dense.g32[0].double(), dense.g64[0]
    o_pr, o_g = float((pr32 - pr64).abs().max()), float((g32 - g64)[use].abs().max())
    b_pr, b_g = max(2.5e-6 * float(pr64.abs().max()), 4 * o_pr), max(3e-7, 4 * o_g)
    d_pr, d_g = float((pr - pr64).abs().max()), float((dchi - g64)[use].abs().max())
    print(f"dense scan path: per_res HIP vs fp64 {d_pr:.2e} (oracle fp32 vs fp64 {o_pr:.2e}, bound {b_pr:.2e}, max {float(pr64.max()):.1f}); "
          f"dchi {d_g:.2e} (oracle {o_g:.2e}, bound {b_g:.2e}, max {float(g64.abs().max()):.2e}); "
          f"{int(dense.marginal.sum())} rows at a hinge threshold left out")
    assert d_pr <= b_pr and d_g <= b_g
    # a chi that moves no clashing atom has gradient exactly 0; Adam would turn a rounding residue there into a full-size step
    assert not bool(((g64 == 0) & (dchi != 0))[use].any())
    _timed(t0, "c scan path vs fp64")


# ---- d. the candidate path reproduces the scan path -------------------------------------------------------------------------------
@gpu
def test_candidate_path_losses_are_the_scan_paths(dense, dense_ctx):
    t0 = time.time()
    gb, ctx = dense_ctx
    chi = dense.chi.to(DEV)
    traj, last, losses = ctx.proximal(chi, VTF, TOL, LAMDA, 5)
    pr0 = ctx.clash(chi, VTF, TOL).double()
    keep = (pr0 > pr0.float().mean().double()).unsqueeze(-1)
    z = chi.double() * keep
    losses = losses.cpu().double().numpy()
    for t in range(5):
        x = chi if t == 0 else traj[t - 1]
        pr = ctx.clash(x, VTF, TOL).double()
        want = float((((x.double() - z) ** 2).sum(-1) + LAMDA * pr).mean())
        print(f"step {t}: loss {losses[t]:.9g}, from the scan path {want:.9g}")
        assert abs(losses[t] - want) <= 2e-6 * max(1.0, abs(want)), (t, losses[t], want)
        assert torch.equal(traj[t][~keep.expand(-1, -1, 4)], chi[~keep.expand(-1, -1, 4)]), t
    assert torch.equal(last, traj[-1]) and not torch.equal(last, chi)
    assert torch.equal(keep[0, :, 0].cpu(), dense.mask64[0, :, 0])
    _timed(t0, "d candidate vs scan losses")


# ---- e / g. packs, pins, and the scan switch of the diagnostic library ------------------------------------------------------------
def _pack_inputs(dense):
    """([45-row synth, dense_complex(), 70-row synth] on the host, their angles, fixed [N]: a third of the ball rows)."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    bs = [protein_to_batch(synth.make_complex(45, 1645)), dense.b, protein_to_batch(synth.make_complex(70, 1670))]
    chis = [start_angles(bs[0], 45), dense.chi, start_angles(bs[2], 70)]
    fixed = torch.zeros(45 + DENSE_L + 70, dtype=torch.bool)
    fixed[45 + torch.from_numpy(BALL_ROWS[::3])] = True
    return bs, chis, fixed


def _three_runs(dense):
    """{name: (traj, last, accepted or None, losses)} of dense_complex() alone, the pack, and the pinned pack."""
    from packppi_amd.batch import pack
    from packppi_amd.functional import _ctx_for, proximal_optimizer_packed
    bs, chis, fixed = _pack_inputs(dense)
    gbs = [b.to(DEV) for b in bs]
    solo = _ctx_for(gbs[1]).proximal(chis[1].to(DEV), VTF, TOL, LAMDA, 5)
    pb = pack(gbs)
    x = torch.cat(chis, 1).to(DEV)
    packed = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, 5, want_traj=True)
    pinned = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, 5, want_traj=True, fixed_mask=fixed.to(DEV))
    free = proximal_optimizer_packed(pb, x, VTF, TOL, LAMDA, 5, want_traj=True, fixed_mask=torch.zeros_like(fixed).to(DEV))
    return dict(solo=(solo[0], solo[1], None, solo[2]), packed=packed, pinned=pinned, free=free), x, fixed


def _print_hashes():
    """Child process of test_candidates_against_scan_bit_for_bit: sha256 of traj, last and losses of the three runs."""
    runs, _, _ = _three_runs(_Dense())
    for name in ("solo", "packed", "pinned"):
        traj, last, _, losses = runs[name]
        h = hashlib.sha256(traj.cpu().numpy().tobytes() + last.cpu().numpy().tobytes() + losses.cpu().numpy().tobytes()).hexdigest()
        print("hash", name, h)


@gpu
def test_candidates_against_scan_bit_for_bit():
    """PP_CLASH_SCAN=1 (diagnostic library, read once per process) makes every wave of the proximal loop scan: the lists are only a
    shortcut to the same partners in the same order, so the three runs must give the same bits either way."""
    from packppi_amd.build import diag_variant_path
    if not os.path.exists(diag_variant_path()):
        pytest.skip("libpackppi_hip.dbg.so not built (__graft_entry__.build() builds it)")
    t0 = time.time()
    code = "import sys; sys.path.insert(0, %r)\nfrom tests import test_clash_capacity as T\nT._print_hashes()\n" % ROOT
    outs = []
    for scan in ("0", "1"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PP_CLASH_SCAN=scan, PACKPPI_LIB=diag_variant_path()),
                           cwd=ROOT, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append([ln for ln in r.stdout.splitlines() if ln.startswith("hash ")])
    assert len(outs[0]) == 3 and outs[0] == outs[1], outs
    _timed(t0, "e candidates vs scan bits")


@gpu
def test_dense_segment_in_a_pack_and_under_an_empty_pin(dense):
    """test_packed_proximal's and test_pinned_proximal's properties on a segment whose waves are in all three regimes."""
    t0 = time.time()
    runs, x, fixed = _three_runs(dense)
    straj, slast, _, slosses = runs["solo"]
    traj, last, acc, losses = runs["packed"]
    a, e = 45, 45 + DENSE_L
    assert torch.equal(losses[1], slosses)
    assert torch.equal(traj[:, :, a:e], straj) and torch.equal(last[:, a:e], slast)
    ls = [float(v) for v in slosses.cpu()]
    assert torch.equal(acc[:, a:e], slast if ls[-1] < ls[0] else dense.chi.to(DEV))
    for k, name in enumerate(("traj", "last", "accepted", "losses")):
        assert torch.equal(runs["free"][k], runs["packed"][k]), name
    # the pin bites: fixed rows keep their bits, and the run is another one
    ptraj, plast, _, _ = runs["pinned"]
    fx = fixed.to(DEV)
    assert all(torch.equal(ptraj[t][0, fx], x[0, fx]) for t in range(5)) and not torch.equal(plast, last)
    assert (last[0, fx] != x[0, fx]).any()
    _timed(t0, "g pack and pin")


# ---- f. against the reference optimiser -------------------------------------------------------------------------------------------
@gpu
def test_three_steps_against_the_reference_optimiser(dense, dense_ctx):
    """test_against_the_restated_reference's idiom: losses rtol 5e-5 against the fp32 reference, angles within
    max(2e-5, 8 x |ref32 - ref64|) per step, on the entries whose first fp64 gradient is at least 1e-5 (below that Adam's first
    step, lr x g / (|g| + eps), is decided by rounding)."""
    t0 = time.time()
    gb, ctx = dense_ctx
    traj, last, losses = ctx.proximal(dense.chi.to(DEV), VTF, TOL, LAMDA, 3)
    losses = losses.cpu().double().numpy()
    (c32, l32), (c64, l64) = dense.ref32, dense.ref64
    rel = np.abs(losses / np.array(l32) - 1).max()
    firm = dense.mask64 & dense.b.SC_D_mask.bool() & (dense.g0 >= 1e-5)
    div = np.array([float(wrapped_absdiff(a, c)[firm].max()) for a, c in zip(c32, c64)])
    d = np.array([float(wrapped_absdiff(traj[t].cpu(), c32[t])[firm].max()) for t in range(3)])
    d64 = np.array([float(wrapped_absdiff(traj[t].cpu(), c64[t])[firm].max()) for t in range(3)])
    env = np.maximum(2e-5, 8 * div)
    print(f"dense proximal: loss rel vs fp32 {rel:.2e} (vs fp64 {np.abs(losses / np.array(l64) - 1).max():.2e}); angles vs fp32 "
          + " ".join(f"{v:.1e}" for v in d) + "; vs fp64 " + " ".join(f"{v:.1e}" for v in d64) + "; reference fp32 vs fp64 "
          + " ".join(f"{v:.1e}" for v in div) + f"; {int(firm.sum())} entries compared")
    assert np.allclose(losses, np.array(l32), rtol=5e-5, atol=1e-7), rel
    assert (d <= env).all(), (d.tolist(), env.tolist())
    still = ~dense.mask64[0, :, 0]
    assert all(torch.equal(traj[t].cpu()[0, still], dense.chi[0, still]) for t in range(3))
    _timed(t0, "f reference optimiser")


# ---- h. the drain-and-resume path -------------------------------------------------------------------------------------------------
def cloud_reference(b, chi, rows, dtype):
    """(per_res [len(rows)], dchi [len(rows), 4]) of the cloud's `rows` from the oracle on the pairs (i, j) for all j."""
    from oracle import ref_cpu as O
    from packppi_amd import constants as rc
    L = CLOUD_L
    X, S, BB = b.X[0].to(dtype), b.residue_type[0], b.BB_D[0].to(dtype)
    ex, ri = b.atom_mask[0].to(dtype), b.residue_index[0]
    chi = chi[0].to(dtype)
    nsc = ex[:, 4:].sum(-1)
    lo, up = rc.make_atom14_dists_bounds(overlap_tolerance=TOL, bond_length_tolerance_factor=VTF)
    radius = ex * torch.as_tensor(rc.between_radius, dtype=dtype)[S]
    with torch.no_grad():
        xyz_all = O.atom14_coords(X, S, BB, chi)                                            # [L, 14, 3]
    out_pr, out_g = [], []
    for i in rows:
        xi = chi[i].clone().requires_grad_(True)
        own = O.atom14_coords(X[i:i + 1], S[i:i + 1], BB[i:i + 1], xi[None])               # [1, 14, 3]
        pair_xyz = torch.stack([own.expand(L, 14, 3), xyz_all], 1)                          # [L, 2, 14, 3]
        pair = lambda v: torch.stack([v[i].expand(L, *v.shape[1:]), v], 1)
        per_atom = O.between_residue_clash(pair_xyz, pair(ex), pair(radius), pair(ri), TOL)  # [L, 2, 14]
        within = O.within_residue_violation(own, ex[i:i + 1], torch.as_tensor(lo, dtype=dtype)[S[i:i + 1]],
                                            torch.as_tensor(up, dtype=dtype)[S[i:i + 1]])
        pr_i = (per_atom[:, 0, 4:].sum() + within[0, 4:].sum()) / (1e-10 + nsc[i])
        partners = (per_atom[:, 1, 4:].sum(-1) / (1e-10 + nsc)).sum()
        ((pr_i + partners) / L).backward()
        out_pr.append(pr_i.detach())
        out_g.append(xi.grad.detach())
    return torch.stack(out_pr), torch.stack(out_g)


def cloud_hinge_allowance(b, chi, rows):
    """(allowance [len(rows), 4], window, rows concerned): how far d(mean clash)/dchi of the sampled rows can jump because a
    between-residue hinge r_a + r_b - tol - d sits within `window` of 0 in fp64, where fp32 may have it on the other side.  Such a pair
    (a of row i, b of row j) switches a force of (w_i [a side chain] + w_j [b side chain]) along the unit vector between the atoms on
    or off: |.| x |unit . dp_a/dchi_k| on chi_k.  The window is what fp32 coordinates can move a distance by: twice (two atoms) the
    largest distance between the oracle's own fp32 and fp64 atom positions on this input -- the reference's error, nothing of the
    kernel's."""
    from oracle import ref_cpu as O
    from packppi_amd import constants as rc
    S = b.residue_type[0]
    X64, BB64, chi64 = b.X[0].double(), b.BB_D[0].double(), chi[0].double()
    with torch.no_grad():
        xyz32 = O.atom14_coords(b.X[0], S, b.BB_D[0], chi[0])
        xyz = O.atom14_coords(X64, S, BB64, chi64)
    ex = b.atom_mask[0].double()
    window = 2 * float(((xyz32.double() - xyz) * ex[..., None]).norm(dim=-1).max())
    r = ex * torch.as_tensor(rc.between_radius, dtype=torch.float64)[S]
    w = (1.0 / CLOUD_L) / (1e-10 + ex[:, 4:].sum(-1))
    bbm = torch.zeros(14, 14, dtype=torch.bool)
    bbm[:4, :4] = True
    bbm[5, 5] = True
    allow, concerned = torch.zeros(len(rows), 4, dtype=torch.float64), 0
    flat, sq = xyz.reshape(-1, 3), (xyz ** 2).sum(-1).reshape(-1)
    for n, i in enumerate(rows):
        # all distances of the row's atoms as |p|^2 + |q|^2 - 2 p.q (fp64: good to 1e-13 A here), the few hits again from the differences
        d = torch.sqrt(1e-10 + (sq[None] + (xyz[i] ** 2).sum(-1)[:, None] - 2 * xyz[i] @ flat.T).clamp(min=0)).reshape(14, CLOUD_L, 14)
        m = ((r[i][:, None, None] * r[None]) != 0) & ~bbm[:, None, :]
        m[:, i] = False
        hits = torch.nonzero(m & ((r[i][:, None, None] + r[None] - TOL - d).abs() < window))
        if len(hits) == 0:
            continue
        concerned += 1
        # dp_a / dchi_k [14, 3, 4] by central differences in fp64 (one batched reconstruction; good to ~1e-9, this is an allowance)
        step = 1e-6 * torch.cat([torch.eye(4, dtype=torch.float64), -torch.eye(4, dtype=torch.float64)])
        with torch.no_grad():
            p8 = O.atom14_coords(X64[i].expand(8, 14, 3), S[i].expand(8), BB64[i].expand(8, 3), chi64[i] + step)
        J = ((p8[:4] - p8[4:]) / 2e-6).permute(1, 2, 0)
        for a, j, bb in hits.tolist():
            cw = (float(w[i]) if a >= 4 else 0.0) + (float(w[j]) if bb >= 4 else 0.0)
            u = xyz[i, a] - xyz[j, bb]
            allow[n] += cw * ((u / u.norm()) @ J[a]).abs()
    return allow, window, concerned


@gpu
def test_drain_and_resume_on_the_collapsed_cloud(cloud):
    """pp_clash with gradient on the cloud: every wave lists 2048 (or 2047) partners, drains them and resumes its scan for the last 32.
    64 rows spread over the four waves' windows against the oracle on the pairs (i, j) for all j, in fp64; bounds as in
    test_scan_path_against_fp64, the project bars scaled by max |value|.  The gradient is discontinuous at a hinge's threshold here
    too, and with 1.6 M atom pairs per row most rows own a pair within fp32 rounding of it (3e-6 A): instead of leaving those rows out,
    every chi entry gets the size of the jumps its row's marginal pairs can cause on top of the bound (cloud_hinge_allowance; zero for
    the other entries), and the oracle's own fp32-to-fp64 distance is taken beyond the same allowance.  Measured without it: 63 rows
    within 1.6e-6, and row 3037 off by 4.0e-5 -- one hinge 5.8e-8 A below its threshold in fp64 and above it on the device; switching
    that one pair on in the fp64 result reproduces the device's gradient to 1.2e-7."""
    from packppi_amd.functional import _ctx_for
    t0 = time.time()
    b, chi = cloud
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    rows = [int(r) for r in np.linspace(0, CLOUD_L - 1, 64).astype(int)]
    assert {(r // 64) % WAVES for r in rows} == {0, 1, 2, 3}
    pr32, g32 = cloud_reference(b, chi, rows, torch.float32)
    pr64, g64 = cloud_reference(b, chi, rows, torch.float64)
    allow, window, concerned = cloud_hinge_allowance(b, chi, rows)
    gb = b.to(DEV)
    ctx = _ctx_for(gb)
    pr, dchi = ctx.clash(chi.to(DEV), VTF, TOL, need_grad=True)
    pr2, dchi2 = ctx.clash(chi.to(DEV), VTF, TOL, need_grad=True)
    assert torch.equal(pr, pr2) and torch.equal(dchi, dchi2)
    assert bool(torch.isfinite(pr).all()) and bool(torch.isfinite(dchi).all())
    pr, dchi = pr.cpu().double()[0, rows], dchi.cpu().double()[0, rows]
    o_pr = float((pr32.double() - pr64).abs().max())
    o_g = float(((g32.double() - g64).abs() - allow).clamp(min=0).max())
    b_pr = max(2.5e-6 * float(pr64.abs().max()), 4 * o_pr)
    b_g = max(3e-7 * float(g64.abs().max()), 4 * o_g)
    d_pr, excess = float((pr - pr64).abs().max()), ((dchi - g64).abs() - allow).clamp(min=0)
    clean = allow == 0
    print(f"collapsed cloud: per_res HIP vs fp64 {d_pr:.2e} (oracle fp32 vs fp64 {o_pr:.2e}, bound {b_pr:.2e}, max {float(pr64.max()):.1f}); "
          f"dchi beyond the hinge allowance {float(excess.max()):.2e} (oracle {o_g:.2e}, bound {b_g:.2e}, max |dchi| {float(g64.abs().max()):.2e}); "
          f"{concerned} of 64 rows own a pair within {window:.2e} A of its threshold, allowance up to {float(allow.max()):.2e}, "
          f"{int(clean.sum())} of 256 entries without; plain distance HIP {float((dchi - g64).abs().max()):.2e}, oracle fp32 "
          f"{float((g32.double() - g64).abs().max()):.2e}, HIP on the entries without allowance {float((dchi - g64).abs()[clean].max()):.2e}")
    assert d_pr <= b_pr and float(excess.max()) <= b_g
    assert int(clean.sum()) >= 64                          # and the comparison is not all allowance
    _timed(t0, "h drain and resume")


# ---- the dbg-only tests, once, on the diagnostic library --------------------------------------------------------------------------
@gpu
def test_diag_library_runs_the_capacity_tests():
    """One child run of the test that reads the device tables on libpackppi_hip.dbg.so (it skips on the product library)."""
    from packppi_amd.build import diag_variant_path
    if os.environ.get("PACKPPI_LIB"):
        pytest.skip("already a child run")
    lib = diag_variant_path()
    if not os.path.exists(lib):
        pytest.skip("libpackppi_hip.dbg.so not built (__graft_entry__.build() builds it)")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "test_clash_capacity.py"), "-q", "-x", "-s", "-m", "gpu",
                        "-p", "no:cacheprovider", "-k", "test_device_extents_and_candidate_counts"],
                       env=dict(os.environ, PACKPPI_LIB=lib), cwd=ROOT, capture_output=True, text=True, timeout=300)
    print(r.stdout[-1500:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-1000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout.splitlines()[-1], r.stdout[-500:]
