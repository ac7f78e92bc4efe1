"""All-atom chi refinement on the device, through the C ABI (pp_chi_refine).

Reference: tests/refine_oracle.py (brute force, no row filter, no partner cap, its own list of the atoms that move).  The candidates
of the first sweep must have the BYTES of ``Context.atom14`` / ``Context.hydrogens`` at the candidate angles, and lie within 1e-5 A +
2 ulp32(largest |coordinate|) of the float64 oracle.  ``steps``, ``chi``, ``e``, ``energy``, ``cand_mask``, ``trace``, ``sweeps``,
``converged`` and ``hmask`` must have the bytes of the float32 restatement, which gets its coordinates from the device's own
``atom14`` / ``hydrogens`` at the angles of its own state.  Nothing measured on the device enters a bound.  The big fixtures run few
sweeps (the restatement costs a millisecond per energy); convergence is checked on the small and the hand-built ones."""
import functools

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc

from . import allatom_oracle as A
from . import polar_oracle as O
from . import refine_oracle as R
from .test_allatom_gpu import _pack3, _padded, arrays, hxyz_tolerance, new_ctx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORDS = ("steps", "e", "energy", "cand_mask", "trace", "sweeps", "converged")


def seeded_chi(b, seed=11, amp=0.35):
    g = torch.Generator().manual_seed(seed)
    chi = b["SC_D"].clone().float()
    return torch.remainder(chi + amp * torch.randn(chi.shape, generator=g) + np.pi, 2 * np.pi) - np.pi


def host(t, *shape):
    return None if t is None else t.reshape(*shape).cpu().numpy()


def words(res, r=0):
    n = res.chi.numel() // 4
    return dict(steps=host(res.steps[r], n, 4), e=host(res.e_round[r], n, 2), energy=host(res.energy[r], n, 9),
                cand_mask=host(res.cand_mask[r], n), trace=host(res.trace[r], *res.trace.shape[1:]), sweeps=host(res.sweeps[r], -1),
                converged=host(res.converged[r], -1))


def assert_same_words(got, want, what=""):
    for k in WORDS:
        dt = np.int8 if k == "steps" else np.int32
        assert got[k].dtype == dt and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].astype(dt).tobytes(), (what, k, int((got[k] != want[k]).sum()))


def device_build(ctx, link=None):
    """The oracle's ``build`` on the device: ``Context.hydrogens`` (atom14 inside) at the angles asked for."""
    n = ctx.B * ctx.L

    def build(chi, rows):
        h = ctx.hydrogens(chi=torch.from_numpy(np.ascontiguousarray(chi)).reshape(ctx.B, ctx.L, 4).to(DEV), link=link)
        return host(h.xyz, n, 14, 3), host(h.hxyz, n, 13, 3), host(h.hmask, n, 13)
    return build


def problem(b, ctx, res, chi, link=None, fixed=None, dtype=np.float32, delta_deg=16.0, **kw):
    _, am, rt, chain, offs = arrays(b)
    n = len(rt)
    lk = None if link is None else np.asarray(torch.as_tensor(link).cpu()).reshape(-1)
    radius = A.default_radius(rt, am, "skip")
    if kw.get("radius") is not None:                           # the caller's radii, the rotatable hydrogens still not counted
        radius = np.where(A.get_tables()["rot"][rt], 0, host(kw["radius"], n, 27)).astype(np.float32)
    kw = {k: v for k, v in kw.items() if k != "radius"}
    return R.Problem(host(chi, n, 4), device_build(ctx, link), rt, chain, offs, host(res.link_prev, n), b["residue_mask"].reshape(-1).numpy(),
                     b["SC_D_mask"].reshape(-1, 4).numpy(), radius, rc.refine_extent, fixed=fixed, link=lk,
                     delta=np.float32(np.deg2rad(delta_deg)), dtype=dtype, **kw)


def check_candidates(ctx, b, res, chi, link=None, what=""):
    """The candidates of the first sweep: the bytes of atom14 / hydrogens at the candidate angles, candidate 0 those at the input, and
    all of them within the bound of the float64 oracle."""
    _, am, rt, chain, offs = arrays(b)
    n = len(rt)
    chi0, cm = host(chi, n, 4).astype(np.float32), host(res.cand_mask[0], n)
    delta = np.float32(res.deltas[0])
    lk = None if link is None else np.asarray(torch.as_tensor(link).cpu()).reshape(-1)
    f64 = R.host_build(b, np.float64, lk)
    worst_h = worst_x = 0.0
    for c in range(R.NCAND):
        st = np.zeros((n, 4), np.int8)
        have = ((cm >> c) & 1) != 0
        if c:
            j, d = R.cand_step(c)
            st[have, j] = d
        ch = R.angles(chi0, st, delta)
        h = ctx.hydrogens(chi=torch.from_numpy(ch).reshape(ctx.B, ctx.L, 4).to(DEV), link=link)
        assert torch.equal(res.cand_xyz[0, c].reshape(-1), h.xyz.reshape(-1)), (what, c)
        assert torch.equal(res.cand_hxyz[0, c].reshape(-1), h.hxyz.reshape(-1)) and torch.equal(res.cand_hmask[0, c].reshape(-1), h.hmask.reshape(-1)), (what, c)
        if c == 0:
            assert ch.tobytes() == chi0.tobytes()
        rows = np.nonzero(have)[0]
        if len(rows) == 0:
            continue
        X64, H64, M64 = f64(ch, rows)
        gx, gh, gm = host(res.cand_xyz[0, c], n, 14, 3), host(res.cand_hxyz[0, c], n, 13, 3), host(res.cand_hmask[0, c], n, 13)
        assert gm[rows].tobytes() == M64[rows].tobytes(), (what, c)
        live = am[rows] != 0
        worst_x = max(worst_x, float(np.abs(gx[rows] - X64[rows])[live].max()))
        # the hydrogens from the device's own heavy atoms, as section 29 bounds them
        Hd, Md, _ = A.hydrogens(gx.astype(np.float64), am, rt, chain, offs, link=lk) if c == 0 else (None, None, None)
        if c == 0:
            worst_h = max(worst_h, float(np.abs(gh - Hd).max()))
    tol = hxyz_tolerance(host(res.cand_xyz[0, 0], n, 14, 3))
    print(f"{what}: candidates: heavy atoms within {worst_x:.3g} A of the float64 reconstruction, hydrogens within {worst_h:.3g} A of the "
          f"float64 placement on the device's heavy atoms (bound {tol:.3g} A)")
    assert worst_h <= tol and worst_x <= tol, (what, worst_x, worst_h, tol)


def run_and_check(b, chi, what, ctx=None, link=None, fixed=None, max_sweeps=4, delta_deg=16.0, ref_kw=None, cands=True, **kw):
    """One call (one round) on the device against the oracle.  ``kw``: for both; ``ref_kw``: what only the oracle is told."""
    ctx = ctx or new_ctx(b)
    chi = chi.to(DEV)
    res = ctx.refine_allatom(chi, fixed=fixed, link=link, deltas_deg=(delta_deg,), max_sweeps=max_sweeps, want_candidates=True, **kw)
    if cands:
        check_candidates(ctx, b, res, chi, link, what)
    p = problem(b, ctx, res, chi, link=link, fixed=fixed, delta_deg=delta_deg, **kw, **(ref_kw or {}))
    ref = R.optimize(p, max_sweeps)
    got = words(res)
    n = len(got["steps"])
    print(f"{what}: movers {len(p.movers)}, with an overlap {len(ref['hot'][0])}, moved {int((got['steps'] != 0).any(1).sum())}, trace "
          f"{ref['trace'][:, 0].tolist()} -> {ref['trace'][:, -1].tolist()}, sweeps {ref['sweeps'].tolist()}, words that differ "
          f"{[int((got[k] != ref[k]).sum()) for k in WORDS]}")
    assert_same_words(got, ref, what)
    assert host(res.chi, n, 4).tobytes() == ref["chi"].tobytes(), what
    # rows that did not move keep the caller's bits; the result reconstructs to its own atoms, bit for bit
    still = ~(got["steps"] != 0).any(1)
    assert host(res.chi, n, 4)[still].tobytes() == host(chi, n, 4)[still].tobytes(), what
    h = ctx.hydrogens(chi=res.chi, link=link)
    assert torch.equal(ctx.atom14(res.chi).reshape(-1), res.xyz.reshape(-1)) and torch.equal(h.hxyz, res.hxyz), what
    assert torch.equal(h.hmask, res.hmask) and torch.equal(h.link_prev, res.link_prev), what
    assert ctx.saturated() == 0
    return ctx, res, ref, p


@functools.lru_cache(maxsize=None)
def solved(name):
    b = CASES[name]()
    return (b,) + run_and_check(b, seeded_chi(b), name, max_sweeps=SWEEPS.get(name, 3))


SINGLES = ("c24", "c64", "c97", "1BRS", "2FTL", "damaged64")
CASES = {**{n: functools.partial(O.batch, n) for n in SINGLES}, "padded": _padded, "pack3": _pack3}
SWEEPS = {"c24": 8, "1BRS": 2, "2FTL": 2, "pack3": 2}


@pytest.mark.parametrize("name", sorted(CASES))
def test_words_against_the_oracle(name):
    b, ctx, res, ref, p = solved(name)
    assert (ref["steps"] != 0).any() and (ref["trace"][:, 0] > ref["trace"][:, -1]).all(), "vacuous: nothing moved"
    tr = ref["trace"].astype(np.int64)
    assert (np.diff(tr, axis=1) <= 0).all()
    for q, acc in enumerate(ref["history"]):
        for s in range(tr.shape[0]):
            assert tr[s, q] - tr[s, q + 1] == sum(g for n, _, g in acc if p.seg_of[n] == s), (name, q, s)
    # a row without an overlap never moved
    ever_hot = set().union(*[set(h) for h in ref["hot"]])
    assert all(n in ever_hot for n in np.nonzero((ref["steps"] != 0).any(1))[0])
    if name == "padded":
        assert not ref["steps"][36 + 40:].any() and (ref["cand_mask"][36 + 40:] == 0).all()
    if name == "1BRS":                                         # no word depends on the energies the oracle took over between sweeps
        again = R.optimize(problem(b, ctx, res, seeded_chi(b)), SWEEPS[name], reuse=False)
        assert all(again[k].tobytes() == ref[k].tobytes() for k in WORDS)


def test_the_same_words_alone_packed_as_a_decoy_and_twice():
    from packppi_amd.batch import replicate
    kw = dict(deltas_deg=(16,), max_sweeps=3, want_candidates=True)
    alone = {}
    for n in ("c97", "c65"):
        b = O.batch(n)
        chi = seeded_chi(b, 7)
        r = new_ctx(b).refine_allatom(chi.to(DEV), **kw)
        alone[n] = (words(r), host(r.chi, -1, 4), host(r.hxyz, -1, 39), chi)
    b = _pack3()
    chi = torch.cat([alone[n][3].reshape(-1, 4) for n in ("c97", "c65", "c97")]).reshape(1, -1, 4)
    ctx = new_ctx(b)
    r1, r2 = ctx.refine_allatom(chi.to(DEV), **kw), ctx.refine_allatom(chi.to(DEV), **kw)
    assert_same_words(words(r1), words(r2), "two runs")
    assert torch.equal(r1.hxyz, r2.hxyz) and torch.equal(r1.xyz, r2.xyz) and torch.equal(r1.chi, r2.chi)
    packed, pc, hx = words(r1), host(r1.chi, -1, 4), host(r1.hxyz, -1, 39)
    for (lo, hi), n, s in (((0, 97), "c97", 0), ((97, 162), "c65", 1), ((162, 259), "c97", 2)):
        for k in ("steps", "e", "energy", "cand_mask"):
            assert packed[k][lo:hi].tobytes() == alone[n][0][k].tobytes(), (n, s, k)
        for k in ("trace", "sweeps", "converged"):
            assert packed[k][s].tobytes() == alone[n][0][k][0].tobytes(), (n, s, k)
        assert pc[lo:hi].tobytes() == alone[n][1].tobytes() and hx[lo:hi].tobytes() == alone[n][2].tobytes()
    bd = replicate(O.batch("c65"), 3)
    rd = new_ctx(bd).refine_allatom(torch.cat([alone["c65"][3].reshape(-1, 4)] * 3).reshape(1, -1, 4).to(DEV), **kw)
    dec = words(rd)
    for d in range(3):
        for k in ("steps", "e", "energy"):
            assert dec[k][65 * d:65 * d + 65].tobytes() == alone["c65"][0][k].tobytes()
        assert dec["trace"][d].tobytes() == alone["c65"][0]["trace"][0].tobytes()


def test_three_decoys_at_three_chi_sets():
    from packppi_amd.batch import replicate
    b = replicate(O.batch("c24"), 3)
    chi = torch.cat([seeded_chi(O.batch("c24"), s).reshape(-1, 4) for s in (1, 2, 3)]).reshape(1, -1, 4)
    ctx, res, ref, p = run_and_check(b, chi, "three decoys", max_sweeps=3)
    assert len({ref["energy"][24 * d:24 * d + 24].tobytes() for d in range(3)}) == 3


@pytest.mark.parametrize("rot_seed,shift", [(None, (1e4, -1e4, 1e4)), (1, (3.0, -7.0, 11.0))])
def test_far_from_the_origin_and_under_a_rotation(rot_seed, shift):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(synth.rigid_motion(O.protein("c24"), rot_seed, np.array(shift)))
    run_and_check(b, seeded_chi(b), f"rotation {rot_seed}, shift {shift}", max_sweeps=3)


@pytest.mark.parametrize("max_sweeps", [0, 1])
def test_few_sweeps(max_sweeps):
    b = O.batch("c24")
    chi = seeded_chi(b)
    ctx, res, ref, p = run_and_check(b, chi, f"max_sweeps {max_sweeps}", max_sweeps=max_sweeps, cands=False)
    assert res.trace.shape == (1, 1, max_sweeps + 1) and int(res.converged[0, 0]) == 0 and int(res.sweeps[0, 0]) == max_sweeps
    if max_sweeps == 0:
        assert not res.steps.any() and torch.equal(res.chi.reshape(-1), chi.to(DEV).reshape(-1))
    else:
        assert int((res.steps != 0).sum()) == len(ref["history"][0]) >= 1 and int(res.steps.abs().max()) == 1


def test_c24_converges_to_a_local_optimum_within_max_steps():
    b = O.batch("c24")
    chi = seeded_chi(b, amp=0.2)
    ctx, res, ref, p = run_and_check(b, chi, "c24 to the end", max_sweeps=96, cands=False)
    assert ref["converged"][0] == 1 and 1 <= ref["sweeps"][0] < 96
    assert np.abs(ref["steps"]).max() == 3, "some chi reached max_steps"
    # no word depends on the energies the oracle took over from the sweep before
    again = R.optimize(problem(b, ctx, res, chi), 96, reuse=False)
    for k in WORDS:
        assert again[k].tobytes() == ref[k].tobytes(), k
    sets = p.candidate_sets(p.movers)
    for n in p.movers:
        e0, _, hot = p.energy(n, p.cur, p.cur_w)
        if hot:
            assert all(p.energy(n, sets[c][1], sets[c][2])[0] >= e0 for c in range(1, R.NCAND) if p.exists(n, c)), n
    one = ctx.refine_allatom(chi.to(DEV), deltas_deg=(16,), max_steps=1, max_sweeps=96)
    assert int(one.steps.abs().max()) == 1 and int(one.converged[0, 0]) == 1


# ---- hand-built cases: obstacle atoms can be put anywhere --------------------------------------------------------------------------------
def lys_row():
    """(batch, row) of a complete lysine of c97."""
    b = O.batch("c97")
    _, am, rt, _, _ = arrays(b)
    t = rc.resname_to_idx["LYS"]
    return b, next(r for r in range(len(rt)) if rt[r] == t and (am[r] != 0).sum() == 9)


def only_moved(ctx, b, rows):
    """Radii that count the moved atoms of ``rows`` alone (the fixtures' own side chains overlap themselves in places)."""
    rt = arrays(b)[2]
    r = torch.zeros_like(ctx.allatom_tables().radius)
    for row in rows:
        moved = R.moved_of_type(int(rt[row]))
        r[row, moved] = ctx.allatom_tables().radius[row, moved]
    return r.reshape(ctx.B, ctx.L, 27)


def test_an_obstacle_on_a_hydrogen_the_lowest_candidate_is_chosen():
    """One lysine, its moved atoms alone counted, a small sphere (0.1 A) 0.3 A beyond HE2.  The energies of the candidates are
    checked against the oracle further down; here the choice must be the lowest of them, the lowest index on ties, the overlap must
    get shallower or go, and a fixed row stays."""
    b, r = lys_row()
    ctx = new_ctx(b)
    chi = b["SC_D"].float().to(DEV)
    rad = only_moved(ctx, b, [r])
    kw = dict(radius=rad, deltas_deg=(16,), want_candidates=True)
    free = ctx.refine_allatom(chi, **kw)
    n = free.chi.numel() // 4
    assert not free.steps.any() and int(free.e[0, r, 0]) <= 0, "alone the lysine has no overlap and stays"
    assert host(free.cand_mask[0], n)[r] == 0x1ff, "a lysine has four chi: nine candidates"
    he = 14 + A.get_tables()["names"][rc.resname_to_idx["LYS"]][14:].index("HE2")
    x = host(free.cand_xyz[0], 9, n, 14, 3)[:, r].astype(np.float64)
    hx = host(free.cand_hxyz[0], 9, n, 13, 3)[:, r].astype(np.float64)
    spot = hx[0, he - 14] + 0.3 * (hx[0, he - 14] - x[0, 8]) / np.linalg.norm(hx[0, he - 14] - x[0, 8])      # 0.3 A beyond HE2, away from CE
    ctx.set_obstacles(torch.tensor([[*spot, 0.1]], dtype=torch.float32))
    res = ctx.refine_allatom(chi, max_sweeps=1, **kw)
    en, e = host(res.energy[0], n, 9)[r], host(res.e, n, 2)[r]
    dist = np.linalg.norm(hx[:, he - 14] - spot, axis=1)
    print("HE2 to the sphere per candidate:", np.round(dist, 3).tolist(), "energies", en.tolist())
    # 0.3 A is inside all four bands of a hydrogen on carbon against the sphere (1.17 + 0.1 - 0.4 = 0.87 A down to 0.42 A)
    gained = en[0] - int(free.energy[0].reshape(n, 9)[r, 0])
    assert gained >= 4 * 64 and gained % 64 == 0
    best = int(np.argmin(en))                                  # the lowest index among equals
    st = host(res.steps[0], n, 4)[r]
    want = np.zeros(4, np.int8)
    if en[best] < en[0]:
        j, d = R.cand_step(best)
        want[j] = d
    assert st.tolist() == want.tolist() and e.tolist()[0] == en[0]
    assert (np.delete(host(res.steps[0], n, 4), r, axis=0) == 0).all()
    full = ctx.refine_allatom(chi, **kw)
    assert int(full.converged[0, 0]) == 1 and int(full.e[0, r, 1]) < int(full.e[0, r, 0])
    tr = host(full.trace[0], -1)
    assert (np.diff(tr.astype(np.int64)) <= 0).all() and tr[0] - tr[-1] == int(full.e[0, r, 0]) - int(full.e[0, r, 1])
    # the same call against the oracle, to the end
    run_and_check(b, chi.cpu(), "lysine with an obstacle", ctx=ctx, radius=rad, max_sweeps=8, cands=False,
                  ref_kw=dict(obst=np.array([[*spot, 0.1]], np.float32), obst_off=[0, 1], r_max=float(rad.max())))
    # fixed: the row stays, whatever overlaps it
    fx = torch.zeros(n, dtype=torch.uint8)
    fx[r] = 1
    held = ctx.refine_allatom(chi, fixed=fx, **kw)
    assert not held.steps.any() and torch.equal(held.chi.reshape(-1), chi.reshape(-1)) and int(held.cand_mask[0].reshape(-1)[r]) == 0


def test_obstacles_against_the_oracle_and_a_polar_one():
    b = O.batch("c64")
    ctx = new_ctx(b)
    chi = seeded_chi(b)
    free = ctx.refine_allatom(chi.to(DEV), deltas_deg=(16,), max_sweeps=0, want_candidates=True)
    n = free.chi.numel() // 4
    rows = np.nonzero(host(free.cand_mask[0], n))[0][:20]
    rng = np.random.default_rng(3)
    xyz = host(free.xyz, n, 14, 3)
    spots = np.concatenate([xyz[rows, 5] + rng.normal(size=(20, 3)) * 2.0, np.full((20, 1), 1.5)], 1).astype(np.float32)
    polar = (np.arange(20) % 2).astype(np.uint8)
    ctx.set_obstacles(torch.from_numpy(spots), polar=polar)
    _, res, ref, _ = run_and_check(b, chi, "c64 with obstacles", ctx=ctx, max_sweeps=3, cands=False,
                                   ref_kw=dict(obst=spots, obst_off=[0, 20], obst_polar=polar))
    assert not np.array_equal(host(res.e_round[0], n, 2)[:, 0], host(free.e_round[0], n, 2)[:, 0])
    _, none, ref0, _ = run_and_check(b, chi, "no polar obstacle", ctx=ctx, max_sweeps=3, cands=False, obst_polar=np.zeros(20, np.uint8),
                                     ref_kw=dict(obst=spots, obst_off=[0, 20]))
    assert not np.array_equal(ref0["e"], ref["e"])


def test_a_fixed_row_inside_a_clash_stays_and_its_partner_moves():
    """A row that won the first sweep against a partner which wanted to move too, and which nobody else held back: fixed, it stays,
    and the partner, whose gain does not depend on a row that stays where it was, moves in its place."""
    b, ctx, res, ref, p = solved("c24")
    g, acc = ref["gains"][0], {n for n, _, _ in ref["history"][0]}
    beats = lambda q, m: g[q] > 0 and not (g[q] < g[m] or (g[q] == g[m] and q > m))
    blockers = {m: [q for q in ref["plist"][m] if beats(q, m)] for m in ref["proposers"][0] if m not in acc}
    partner, mover = next((m, qs[0]) for m, qs in sorted(blockers.items()) if len(qs) == 1 and qs[0] in acc)
    fx = np.zeros(p.N, np.uint8)
    fx[mover] = 1
    _, held, href, _ = run_and_check(b, seeded_chi(b), "a fixed row", ctx=ctx, fixed=torch.from_numpy(fx), max_sweeps=1, cands=False)
    assert ref["steps"][mover].any() and not href["steps"][mover].any() and href["cand_mask"][mover] == 0
    assert href["steps"][partner].any() and partner in {n for n, _, _ in href["history"][0]}


def test_a_bridged_cysteine_stays():
    name = next(nm for nm in ("2FTL", "1BRS", "c97", "c64") if (arrays(O.batch(nm))[2] == rc.resname_to_idx["CYS"]).sum() >= 2)
    b = O.batch(name)
    rt = arrays(b)[2]
    i, j = np.nonzero(rt == rc.resname_to_idx["CYS"])[0][:2]
    link = -np.ones(len(rt), np.int32)
    link[i], link[j] = j, i
    chi = seeded_chi(b)
    ctx, res, ref, p = run_and_check(b, chi, f"{name} with a disulfide", link=torch.from_numpy(link), max_sweeps=2, cands=False)
    cm = host(res.cand_mask[0], -1)
    assert cm[i] == 0 and cm[j] == 0 and (host(res.hmask, -1, 13)[[i, j], 4] == 0).all()
    free = host(ctx.refine_allatom(chi.to(DEV), deltas_deg=(16,), max_sweeps=0, want_candidates=True).cand_mask[0], -1)
    assert free[i] != 0 and free[j] != 0


def test_a_row_over_the_partner_list_capacity_gets_the_words_of_the_oracle():
    from .test_clash_capacity import dense_complex
    b = dense_complex()
    fixed = torch.from_numpy((np.arange(b["residue_type"].numel()) % 3 != 0).astype(np.uint8))       # a third of the rows: the oracle's time
    ctx, res, ref, p = run_and_check(b, b["SC_D"].float(), "dense", fixed=fixed, max_sweeps=1, cands=False)
    n_partners = np.array([len(ref["plist"][r]) for r in sorted(ref["plist"])])
    print(f"dense: {len(n_partners)} movers, {int((n_partners > 16).sum())} of them with more than 16 partners (up to {int(n_partners.max())})")
    assert (n_partners > 16).sum() >= 30 and ref["sweeps"][0] == 1


def test_the_higher_gain_of_two_coupled_movers_moves_first():
    b, ctx, res, ref, p = solved("c24")
    # among the proposers of the first sweep, two partners: the one the rule prefers is in the accepted list, the other is not
    prop = ref["proposers"][0]
    acc = {n for n, _, _ in ref["history"][0]}
    pairs = [(n, m) for n in prop for m in ref["plist"][n] if m in prop and n in acc]
    assert pairs and all(m not in acc for _, m in pairs)
    st = host(res.steps[0], p.N, 4)
    one = ctx.refine_allatom(seeded_chi(b).to(DEV), deltas_deg=(16,), max_sweeps=1)
    moved = set(np.nonzero((host(one.steps[0], p.N, 4) != 0).any(1))[0].tolist())
    assert moved == acc


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------------
def test_chained_rounds_equal_single_calls_and_the_result_goes_on():
    from packppi_amd.functional import refine_allatom
    b = O.batch("c64")
    ctx = new_ctx(b)
    chi = seeded_chi(b).to(DEV)
    res = ctx.refine_allatom(chi, max_sweeps=6)
    cur = chi
    for r, d in enumerate((16, 8, 4)):
        one = ctx.refine_allatom(cur, deltas_deg=(d,), max_sweeps=6)
        assert torch.equal(one.steps[0], res.steps[r]) and torch.equal(one.trace[0], res.trace[r]) and torch.equal(one.e_round[0], res.e_round[r])
        cur = one.chi
    assert torch.equal(cur, res.chi) and torch.equal(one.xyz, res.xyz) and torch.equal(one.hxyz, res.hxyz)
    assert (res.trace[1:, :, 0] == res.trace[:-1, :, -1]).all(), "a round starts at the energy the one before ended with"
    assert torch.equal(res.F[:, 0], res.trace[0, :, 0].long()) and int(res.F[0, 1]) < int(res.F[0, 0])
    assert torch.equal(res.moved, (res.steps != 0).any(-1).any(0)) and int(res.moved.sum()) >= 1
    before, after = ctx.clashscore(chi=chi), ctx.clashscore(chi=res.chi)
    again = ctx.clashscore(hydrogens=res)
    assert torch.equal(after.seg, again.seg) and torch.equal(after.hxyz, res.hxyz)
    print(f"c64: clashscore {float(before.clashscore[0]):.2f} -> {float(after.clashscore[0]):.2f}, F {res.F[0].tolist()}")
    hn = ctx.hbond_optimize(chi=res.chi)
    assert hn.chi is not None
    f = refine_allatom(b.to(DEV), chi, max_sweeps=6)
    assert torch.equal(f.chi, res.chi) and torch.equal(f.steps, res.steps)


def test_refusals():
    from packppi_amd import lib as L
    b = O.batch("c24")
    ctx = new_ctx(b)
    chi = b["SC_D"].float().to(DEV)
    for kw, msg in ((dict(max_sweeps=-1), "max_sweeps"), (dict(max_sweeps=257), "max_sweeps"), (dict(hb_weak=float("nan")), "finite"),
                    (dict(cut=float("inf")), "finite"), (dict(hb_allow=-0.1), "hb_allow"), (dict(hb_good=3.0), "hb_good"),
                    (dict(obst_polar=[1]), "obstacle"), (dict(radius=torch.zeros(5)), "radius"), (dict(bands=0), "bands"),
                    (dict(bands=9), "bands"), (dict(band=0.0), "band"), (dict(deltas_deg=()), "deltas_deg"), (dict(deltas_deg=(0,)), "deltas_deg"),
                    (dict(max_steps=0), "max_steps"), (dict(deltas_deg=(70,), max_steps=3), "180"), (dict(fixed=np.zeros(3)), "fixed")):
        with pytest.raises(ValueError, match=msg):
            ctx.refine_allatom(chi, **kw)
    with pytest.raises(ValueError, match="link"):
        ctx.refine_allatom(chi, link=np.zeros(3, np.int32))
    # the C entry itself
    res = ctx.refine_allatom(chi, deltas_deg=(16,), max_sweeps=4)
    tabs = ctx.allatom_tables()
    lib, ptr = L.load(), L._ptr
    f32 = np.float32
    n = 24

    def call(**over):
        new = lambda *s, dt=torch.float32: torch.empty(*s, dtype=dt, device=DEV)
        a = dict(chi0=chi, fixed=None, place=tabs.place, param=tabs.param, ext=ctx._rf_ext, radius=res.radius, acls=tabs.acls,
                 aa_sep=tabs.aa_sep, link=None, obst_polar=None, delta=float(f32(np.deg2rad(16.0))), max_steps=3, bands=4, band=0.15, cut=0.4,
                 hb_allow=0.6, hb_weak=2.5, hb_weak2=float(f32(2.5) * f32(2.5)), hb_good2=float(f32(2.2) * f32(2.2)), reach=3.2, max_sweeps=4,
                 chi_out=new(n, 4), steps=new(n, 4, dt=torch.int8), xyz_out=new(n, 42), hxyz_out=new(n, 39), hmask_out=new(n, 13, dt=torch.uint8),
                 link_prev=new(n, dt=torch.uint8), e=new(n, 2, dt=torch.int32), trace=new(1, 5, dt=torch.int32), sweeps=new(1, dt=torch.int32),
                 converged=new(1, dt=torch.int32), cand_xyz=None, cand_hxyz=None, cand_hmask=None, cand_mask=None, energy=None)
        a.update(over)
        args = [ptr(v) if (isinstance(v, torch.Tensor) or v is None) else v for v in a.values()]
        return lib.pp_chi_refine(ctx.handle, *args, ctx._stream()), a

    rc_, a = call()
    assert rc_ == 0 and torch.equal(a["steps"].reshape(-1), res.steps.reshape(-1)) and torch.equal(a["chi_out"].reshape(-1), res.chi.reshape(-1))
    for k in ("chi0", "place", "param", "ext", "radius", "acls", "aa_sep", "chi_out", "steps", "xyz_out", "hxyz_out", "hmask_out", "link_prev",
              "e", "trace", "sweeps", "converged"):
        assert call(**{k: None})[0] == 1 and b"pp_chi_refine" in lib.pp_last_error(), k
    some = torch.empty(9 * n * 42, device=DEV)
    for over in (dict(cand_xyz=some), dict(cand_mask=a["sweeps"]), dict(delta=0.0), dict(delta=float("nan")), dict(max_steps=0),
                 dict(max_steps=17), dict(delta=1.2), dict(bands=0), dict(bands=9), dict(band=0.0), dict(band=float("inf")),
                 dict(cut=float("nan")), dict(hb_allow=-1.0), dict(hb_weak=0.0), dict(hb_weak2=float("nan")), dict(hb_good2=-1.0),
                 dict(hb_good2=7.0), dict(reach=float("inf")), dict(reach=1.0), dict(max_sweeps=-1), dict(max_sweeps=257),
                 dict(obst_polar=a["hmask_out"])):
        assert call(**over)[0] == 1 and b"pp_chi_refine" in lib.pp_last_error(), over
    assert ctx.saturated() == 0


def test_a_bad_table_entry_is_found_on_the_device():
    """A ``place`` entry outside its range: pp_hydrogens, which the entry runs, drops the hydrogen and sets bit 3; the refinement
    never uses the entry as an index and counts no such hydrogen."""
    from packppi_amd import lib as L
    b = O.batch("c24")
    ctx = new_ctx(b)
    chi = seeded_chi(b).to(DEV)
    tabs = ctx.allatom_tables()
    rt = arrays(b)[2]
    t = int(rt[np.nonzero(host(ctx.refine_allatom(chi, deltas_deg=(16,), max_sweeps=0, want_candidates=True).cand_mask[0], -1))[0][0]])
    k = int(np.nonzero(rc.hydrogen_place[t, :, 1] >= 4)[0][0])
    place = rc.hydrogen_place.copy()
    place[t, k, 1] = 15
    good = tabs.place
    tabs["place"] = torch.from_numpy(place).to(DEV)
    try:
        res = ctx.refine_allatom(chi, deltas_deg=(16,), max_sweeps=2)
    finally:
        tabs["place"] = good
    assert ctx.saturated() == 8
    assert (host(res.hmask, -1, 13)[rt == t, k] == 0).all()


def test_the_keyword_on_the_module(weights):
    from packppi_amd.module import TDiffusionModule
    model = TDiffusionModule(weights, device=DEV)
    model.schedule = torch.linspace(1, 0, 4)
    b = O.batch("c64")
    gb = b.to(DEV)
    plain = model.sample_ensemble(gb, 3, seed=11, return_all=True)
    out = model.sample_ensemble(gb, 3, seed=11, return_all=True, refine_allatom=True)
    assert set(out) - set(plain) == {"refine_moved", "refine_F"}
    (chi0, packed), (chi1, _) = plain["decoys"], out["decoys"]
    res = new_ctx(packed).refine_allatom(chi0)
    assert torch.equal(res.chi, chi1) and not torch.equal(chi0, chi1)
    assert out["refine_moved"].shape == (3,) and torch.equal(out["refine_moved"], res.moved.reshape(3, -1).sum(1)) and int(out["refine_moved"].min()) >= 1
    assert out["refine_F"].shape == (3, 2) and torch.equal(out["refine_F"], res.F) and bool((out["refine_F"][:, 1] < out["refine_F"][:, 0]).all())
    # one complex: behind the sampler; kept rows stay kept
    a, r = model.sampling(gb, seed=11), model.sampling(gb, seed=11, refine_allatom=True)
    assert torch.equal(r, new_ctx(b).refine_allatom(a).chi) and not torch.equal(a, r)
    fixed = (torch.arange(64) % 2 == 0).reshape(1, 64)
    k0, k1 = model.repack(gb, fixed, seed=11), model.repack(gb, fixed, seed=11, refine_allatom=True)
    assert torch.equal(k1[fixed.to(DEV)], k0[fixed.to(DEV)]) and not torch.equal(k1, k0)
    assert torch.equal(k1, new_ctx(b).refine_allatom(k0, fixed=fixed).chi)
    with pytest.raises(ValueError, match="refine_allatom"):
        model.sampling(gb, seed=11, refine_allatom=True, return_trajectory=True)


def _files(plain, flagged, extra):
    """``flagged`` holds every file of ``plain`` and exactly the ``extra`` names more; returns the common files whose bytes differ."""
    a, b = {p.name for p in plain.iterdir()}, {p.name for p in flagged.iterdir()}
    assert b - a == set(extra) and a <= b, (sorted(a), sorted(b))
    return [n for n in sorted(a) if (plain / n).read_bytes() != (flagged / n).read_bytes()]


def test_eval_diffusion_with_and_without_the_flag(tmp_path, capsys):
    from packppi_amd import synth
    from packppi_amd.analysis import REFINE_CSV_HEADER, refine_csv
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    src = str(tmp_path / "in.pdb")
    with open(src, "w") as fh:
        fh.write(to_pdb(synth.make_complex(64, 11)))
    base = ["--input", src, "--molprobity_clash_loc", "none", "--random_weights", "0", "--seed", "7", "--steps", "3", "--device", DEV]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    eval_diffusion.main(base + ["--outdir", str(plain), "--clashscore"])
    assert "all-atom refinement" not in capsys.readouterr().out
    eval_diffusion.main(base + ["--outdir", str(flagged), "--clashscore", "--refine_allatom"])
    text = capsys.readouterr().out
    assert set(_files(plain, flagged, ["refine.csv"])) == {"structure.pdb", "clashes.csv"}
    protein = from_pdb_file(src)
    b = protein_to_batch(protein).to(DEV)
    args = eval_diffusion.parse_args(base + ["--outdir", str(tmp_path / "again")])
    chi = eval_diffusion.load_model(args).sampling(b, seed=7)
    ctx = new_ctx(b)
    res = ctx.refine_allatom(chi)
    got = (flagged / "refine.csv").read_text()
    assert got == refine_csv(protein["aaindex"], res.steps[:, 0].cpu().numpy(), (16, 8, 4), res.e[0].cpu().numpy(), protein["chain_id"],
                             protein["residue_index"])
    assert got.startswith(REFINE_CSV_HEADER + "\n") and len(got.splitlines()) == 1 + int(res.moved.sum()) >= 2
    F = res.F[0].tolist()
    assert f"all-atom refinement: energy {F[0]} -> {F[1]}, sweeps per round {res.sweeps[:, 0].tolist()}" in text
    before, after = ctx.clashscore(chi=chi), ctx.clashscore(chi=res.chi)
    assert (f"clashscore {float(before.clashscore[0]):.2f} before, {float(after.clashscore[0]):.2f} after the all-atom refinement "
            f"(--refine_allatom)") in text
    c = from_pdb_file(flagged / "structure.pdb")
    m = c["atom_mask"] != 0
    assert np.abs(c["atom_positions"][m] - np.round(res.xyz[0].cpu().numpy().astype(np.float64), 3)[:len(m)][m]).max() <= 1.5e-3
    # decoys: ensemble.csv gains the columns, refine.csv appears
    e0, e1 = tmp_path / "ens0", tmp_path / "ens1"
    eval_diffusion.main(base + ["--outdir", str(e0), "--n_decoys", "2"])
    eval_diffusion.main(base + ["--outdir", str(e1), "--n_decoys", "2", "--refine_allatom"])
    assert "ensemble.csv" in _files(e0, e1, ["refine.csv"])
    r0 = [ln.split(",") for ln in (e0 / "ensemble.csv").read_text().strip().split("\n")]
    r1 = [ln.split(",") for ln in (e1 / "ensemble.csv").read_text().strip().split("\n")]
    assert r1[0] == r0[0] + ["refine_moved", "refine_F_before", "refine_F_after"] and len(r1) == 3
    assert all(int(r[-3]) >= 1 and int(r[-1]) < int(r[-2]) for r in r1[1:])


def test_mutate_and_proximal_optimize_with_and_without_the_flag(tmp_path, capsys):
    from packppi_amd.analysis import REFINE_CSV_HEADER
    from packppi_amd.cli import mutate, proximal_optimize
    from packppi_amd.pdb_io import to_pdb
    pdb = tmp_path / "1brs.pdb"
    pdb.write_text(to_pdb(O.protein("1BRS")))
    base = ["--input", str(pdb), "--mutstr", "LA87F", "--device", "cuda", "--random_weights", "3", "--steps", "3", "--seed", "7",
            "--n_decoys", "2"]
    m0, m1 = tmp_path / "m0", tmp_path / "m1"
    mutate.main(base + ["--outdir", str(m0)])
    mutate.main(base + ["--outdir", str(m1), "--refine_allatom"])
    changed = _files(m0, m1, ["refine_LA87F.csv"])
    assert set(changed) <= {"mutants.csv", "mutant_LA87F.pdb"} and "mutants.csv" in changed
    lines = (m1 / "refine_LA87F.csv").read_text().splitlines()
    assert lines[0] == REFINE_CSV_HEADER
    r0 = [ln.split(",") for ln in (m0 / "mutants.csv").read_text().splitlines()]
    r1 = [ln.split(",") for ln in (m1 / "mutants.csv").read_text().splitlines()]
    assert r1[0] == r0[0] + ["refine_moved", "refine_F_before", "refine_F_after"] and r1[1][0] == r0[1][0]
    assert int(r1[1][-1]) <= int(r1[1][-2])
    assert (int(r1[1][-3]) >= 1) == (len(lines) >= 2), "the selected decoy's moved rows are the lines of its refine csv"
    capsys.readouterr()
    pbase = ["--input", str(pdb), "--molprobity_clash_loc", "none", "--num_steps", "5", "--device", "cuda"]
    p0, p1 = tmp_path / "p0", tmp_path / "p1"
    proximal_optimize.main(pbase + ["--outdir", str(p0), "--clashscore"])
    assert "all-atom refinement" not in capsys.readouterr().out
    proximal_optimize.main(pbase + ["--outdir", str(p1), "--clashscore", "--refine_allatom"])
    out = capsys.readouterr().out
    assert "all-atom refinement: energy " in out and "after the all-atom refinement (--refine_allatom)" in out
    assert set(_files(p0, p1, ["refine.csv"])) == {"structure.pdb", "clashes.csv"}
    text = (p1 / "refine.csv").read_text()
    assert text.startswith(REFINE_CSV_HEADER + "\n") and len(text.splitlines()) >= 2


# ---- hand-built cases on serines: one chi, three candidates, one counted atom ----------------------------------------------------------------
# Only OG (slot 5, radius 1.40 A) of the chosen serines is counted, against obstacle spheres put relative to the device's own candidate
# positions.  Every construction checks its own premise in float64 first: each distance is at least 0.02 A from a band threshold.
SER_PAIR = ("2FTL", 16, 27)            # two complete serines whose CA are 8.75 A apart: partners (3.9 + 3.9 + 3.2 A), too far for a term


def _serines(rows, chi1=None):
    """``chi1``: put the serines' chi1 there first (the construction works at any angle)."""
    b = O.batch(SER_PAIR[0])
    ctx = new_ctx(b)
    rad = torch.zeros_like(ctx.allatom_tables().radius)
    rad[list(rows), 5] = ctx.allatom_tables().radius[list(rows), 5]
    rad = rad.reshape(ctx.B, ctx.L, 27)
    chi = b["SC_D"].float().clone()
    if chi1 is not None:
        chi[0, list(rows), 0] = chi1
    chi = chi.to(DEV)
    free = ctx.refine_allatom(chi, radius=rad, deltas_deg=(16,), max_sweeps=0, want_candidates=True)
    n = chi.numel() // 4
    assert all(int(free.cand_mask[0].reshape(-1)[r]) == 0b111 for r in rows), "a serine has one chi: candidates 0, 1 (+1) and 2 (-1)"
    assert not free.e.any(), "alone the counted atoms have no term"
    xyz = host(free.cand_xyz[0], 9, n, 14, 3).astype(np.float64)
    return b, ctx, chi, rad, n, xyz


def _levels(d, t, bands=4, band=0.15):
    """(level, distance to the nearest band threshold) of a pair at distance d with threshold t, in float64."""
    ts = [t - k * band for k in range(bands)]
    return sum(1 for x in ts if x > 0 and d <= x), min(abs(d - x) for x in ts)


def _beside(xyz, r, dist):
    """The point ``dist`` A from OG of row r at candidate 0, on the side candidate 1 turns to: candidate 2 (-1 step) moves away from it."""
    u = xyz[1, r, 5] - xyz[2, r, 5]
    return xyz[0, r, 5] + dist * u / np.linalg.norm(u)


def _sphere_beside(xyz, r, level, t=1.10):
    """A point beside OG of row r (``_beside``) at which candidate 0 is ``level`` bands deep in a sphere of threshold t, candidate 2
    is clear of it and candidate 1 at least as deep, every distance 0.02 A or more from a band threshold; and the three levels."""
    mid = t - 0.15 * (level - 1) - 0.075
    for dist in (mid, mid - 0.02, mid + 0.02, mid - 0.04, mid + 0.04):
        spot = _beside(xyz, r, dist)
        got = [_levels(float(np.linalg.norm(xyz[c, r, 5] - spot)), t) for c in range(3)]
        if min(g[1] for g in got) >= 0.02:
            break
    lv = [g[0] for g in got]
    assert min(g[1] for g in got) >= 0.02 and lv[0] == level and lv[2] == 0 and lv[1] >= lv[0], got
    return spot, lv


def test_a_single_step_down_clears_the_only_overlap():
    """A sphere of 0.1 A (threshold 1.40 + 0.1 - 0.4 = 1.10 A) about 1.03 A from OG: level 1.  One step down on chi1 takes OG 1.3 A or more
    from it, one step up brings it closer.  Exactly that step is taken, no term of level 1 is left, and the segment converges."""
    name, r, _ = SER_PAIR
    b, ctx, chi, rad, n, xyz = _serines([r])
    spot, lv = _sphere_beside(xyz, r, 1)
    ctx.set_obstacles(torch.tensor([[*spot, 0.1]], dtype=torch.float32))
    res = ctx.refine_allatom(chi, radius=rad, deltas_deg=(16,), want_candidates=True)
    assert host(res.energy[0], n, 9)[r].tolist() == [64, 64 * lv[1], 0, 0, 0, 0, 0, 0, 0]
    st = host(res.steps[0], n, 4)
    assert st[r].tolist() == [-1, 0, 0, 0] and not np.delete(st, r, axis=0).any()
    assert host(res.e, n, 2)[r].tolist() == [64, 0] and res.F[0].tolist() == [64, 0]
    assert int(res.sweeps[0, 0]) == 1 and int(res.converged[0, 0]) == 1 and res.trace[0, 0].tolist() == [64] + [0] * 32
    after = ctx.clashscore(chi=res.chi, radius=rad)
    assert int(after.seg[0, 6]) == 0 and int(ctx.clashscore(chi=chi, radius=rad).seg[0, 6]) == 1, "the serious overlap with the obstacle is gone"
    run_and_check(b, chi.cpu(), "a step that clears", ctx=ctx, radius=rad, max_sweeps=2, cands=False,
                  ref_kw=dict(obst=np.array([[*spot, 0.1]], np.float32), obst_off=[0, 1], r_max=float(rad.max())))


def test_a_step_that_only_makes_the_overlap_shallower_is_taken():
    """A sphere of 50 A is a wall (threshold 1.40 + 50 - 0.4 = 51.0 A): one step down moves OG 0.3 to 0.4 A back from it, which leaves it
    0.05 to 0.10 A deep -- level 1 -- where it was three or four bands deep.  Without graded bands both states would cost 64 and
    nothing would move; with them the step is taken and the level drops but stays at least 1."""
    name, r, _ = SER_PAIR
    b, ctx, chi, rad, n, xyz = _serines([r])
    u = (xyz[1, r, 5] - xyz[2, r, 5]) / np.linalg.norm(xyz[1, r, 5] - xyz[2, r, 5])
    t = 51.0
    for depth2 in (0.075, 0.05, 0.10):                        # the depth left at candidate 2; the first that keeps every margin
        # solve for the centre on the line through candidate 2 along u: candidate 2 is exactly depth2 deep
        centre = xyz[2, r, 5] + (t - depth2) * u
        got = [_levels(float(np.linalg.norm(xyz[c, r, 5] - centre)), t) for c in range(3)]
        if min(g[1] for g in got) >= 0.02:
            break
    lv = [g[0] for g in got]
    assert min(g[1] for g in got) >= 0.02 and lv[2] == 1 and lv[0] >= 2 and lv[1] >= lv[0], got
    ctx.set_obstacles(torch.tensor([[*centre, 50.0]], dtype=torch.float32))
    res = ctx.refine_allatom(chi, radius=rad, deltas_deg=(16,), max_sweeps=1, want_candidates=True)
    assert host(res.energy[0], n, 9)[r, :3].tolist() == [64 * v for v in lv]
    assert host(res.steps[0], n, 4)[r].tolist() == [-1, 0, 0, 0] and int(res.sweeps[0, 0]) == 1
    assert host(res.e, n, 2)[r].tolist() == [64 * lv[0], 64], "the level dropped and is still 1: a serious overlap remains"
    assert int(ctx.clashscore(chi=res.chi, radius=rad).seg[0, 6]) == 1


def test_a_mover_with_an_overlap_that_no_candidate_helps_stays():
    """A sphere centred on the CA-CB axis, at the foot of OG: chi1 turns OG about that axis, so every candidate is as far from the
    centre as the current state (1.3 A; threshold 1.40 + 0.6 - 0.4 = 1.60 A: level 2 or 3 everywhere).  The mover has an overlap,
    no candidate is lower, nothing moves and the segment converges without a sweep."""
    name, r, _ = SER_PAIR
    b, ctx, chi, rad, n, xyz = _serines([r])
    ca, cb, og = xyz[0, r, 1], xyz[0, r, 4], xyz[0, r, 5]
    ax = (cb - ca) / np.linalg.norm(cb - ca)
    foot = ca + ax * float((og - ca) @ ax)
    d = [float(np.linalg.norm(xyz[c, r, 5] - foot)) for c in range(3)]
    lv = [_levels(x, 1.60) for x in d]
    assert max(d) - min(d) < 1e-4 and len({v[0] for v in lv}) == 1 and lv[0][0] >= 1 and min(v[1] for v in lv) >= 0.02, (d, lv)
    ctx.set_obstacles(torch.tensor([[*foot, 0.6]], dtype=torch.float32))
    res = ctx.refine_allatom(chi, radius=rad, deltas_deg=(16,), want_candidates=True)
    en = host(res.energy[0], n, 9)[r]
    assert en[0] == 64 * lv[0][0] and (en[1:3] >= en[0]).all() and int(res.cand_mask[0].reshape(-1)[r]) == 0b111
    assert not res.steps.any() and torch.equal(res.chi.reshape(-1), chi.reshape(-1))
    assert int(res.sweeps[0, 0]) == 0 and int(res.converged[0, 0]) == 1 and host(res.e, n, 2)[r].tolist() == [int(en[0])] * 2
    assert (res.trace[0, 0] == int(en[0])).all()


def test_two_built_partners_the_higher_gain_first_and_a_fixed_one_never():
    """Two serines that are partners, each with a sphere of its own that one step down clears: the lower row one band deep (gain 64),
    the higher row two bands deep (gain 128).  The higher row moves in sweep 1 although the lower one wants to as well, the lower
    row in sweep 2.  With the higher row fixed the lower one moves at once and the fixed one never."""
    name, i, j = SER_PAIR
    b, ctx, chi, rad, n, xyz = _serines([i, j])
    (si, li), (sj, lj) = _sphere_beside(xyz, i, 1), _sphere_beside(xyz, j, 2)
    assert min(np.linalg.norm(xyz[:3, i, 5] - sj, axis=1).min(), np.linalg.norm(xyz[:3, j, 5] - si, axis=1).min()) > 3.0, "each sphere is its row's alone"
    spots = np.array([[*si, 0.1], [*sj, 0.1]], np.float32)
    ctx.set_obstacles(torch.from_numpy(spots))
    kw = dict(radius=rad, deltas_deg=(16,), want_candidates=True)
    one = ctx.refine_allatom(chi, max_sweeps=1, **kw)
    st = host(one.steps[0], n, 4)
    assert st[j].tolist() == [-1, 0, 0, 0] and not st[i].any() and int(one.converged[0, 0]) == 0
    assert host(one.energy[0], n, 9)[[i, j], :3].tolist() == [[64, 64 * li[1], 0], [128, 64 * lj[1], 0]]
    _, res, ref, p = run_and_check(b, chi.cpu(), "two built partners", ctx=ctx, radius=rad, max_sweeps=4, cands=False,
                                   ref_kw=dict(obst=spots, obst_off=[0, 2], r_max=float(rad.max())))
    assert j in ref["plist"][i] and [sorted(n_ for n_, _, _ in a) for a in ref["history"][:2]] == [[j], [i]]
    assert host(res.steps[0], n, 4)[[i, j]].tolist() == [[-1, 0, 0, 0]] * 2 and int(res.sweeps[0, 0]) == 2 and int(res.converged[0, 0]) == 1
    assert res.trace[0, 0, :3].tolist() == [192, 64, 0]
    fx = torch.zeros(n, dtype=torch.uint8)
    fx[j] = 1
    held = ctx.refine_allatom(chi, fixed=fx, max_sweeps=1, **kw)
    st = host(held.steps[0], n, 4)
    assert st[i].tolist() == [-1, 0, 0, 0] and not st[j].any() and int(held.cand_mask[0].reshape(-1)[j]) == 0
    assert torch.equal(held.chi.reshape(-1, 4)[j], chi.reshape(-1, 4)[j])
    # the fixed row's overlap is nobody's term: F holds the free row's alone
    assert held.trace[0, 0].tolist() == [64, 0]


def test_a_step_across_pi_wraps_as_the_oracle_wraps():
    """The clearing step of the first case with the serine's chi1 at -3.1: one step down is -3.379, which the entry returns as
    -3.379 + 2 pi in [-pi, pi), the float32 word of the restatement; the candidates on either side of the branch cut have the bytes of
    atom14 / hydrogens at the wrapped angles (``check_candidates``), and the result reconstructs to its own atoms."""
    name, r, _ = SER_PAIR
    b, ctx, chi, rad, n, xyz = _serines([r], chi1=-3.1)
    spot, lv = _sphere_beside(xyz, r, 1)
    ctx.set_obstacles(torch.tensor([[*spot, 0.1]], dtype=torch.float32))
    _, res, ref, _ = run_and_check(b, chi.cpu(), "a step across -pi", ctx=ctx, radius=rad, max_sweeps=2,
                                   ref_kw=dict(obst=np.array([[*spot, 0.1]], np.float32), obst_off=[0, 1], r_max=float(rad.max())))
    assert host(res.steps[0], n, 4)[r].tolist() == [-1, 0, 0, 0]
    got = host(res.chi, n, 4)[r, 0]
    d = np.float32(np.deg2rad(16.0))
    assert got.tobytes() == np.float32(np.float32(np.float32(-3.1) + np.float32(-1.0) * d) + R.TWO_PI).tobytes() and 2.8 < got < 3.0


def test_eval_diffusion_with_obstacles_the_ligand_atoms_count(tmp_path, capsys):
    """--refine_allatom with --obstacles hetero: refine.csv is the text of a call on a context that holds the ligand atoms, and the
    energies of that call are not those of the same call without them."""
    from packppi_amd import synth
    from packppi_amd.analysis import refine_csv
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, insert_obstacle_lines, obstacle_atoms, to_pdb
    from .test_obstacles_host import _rec
    from .test_sasa_host import ligand_near
    prot = synth.make_complex(48, 5)
    lig = ligand_near(protein_to_batch(prot), 9, 3)
    het = [_rec("HETATM", 900 + k, f" C{k + 1} ", " ", "LIG", "A", 301, float(q[0]), float(q[1]), float(q[2]), 1.0, "C") for k, q in enumerate(lig)]
    src = str(tmp_path / "in.pdb")
    with open(src, "w") as fh:
        fh.write(insert_obstacle_lines(to_pdb(prot), het))
    base = ["--input", src, "--molprobity_clash_loc", "none", "--random_weights", "0", "--seed", "7", "--steps", "3", "--device", DEV,
            "--obstacles", "hetero"]
    out = tmp_path / "out"
    eval_diffusion.main(base + ["--outdir", str(out), "--refine_allatom"])
    protein = from_pdb_file(src)
    b = protein_to_batch(protein, obstacles=obstacle_atoms(src))
    args = eval_diffusion.parse_args(base + ["--outdir", str(tmp_path / "again")])
    chi = eval_diffusion.load_model(args).sampling(b.to(DEV), seed=7)
    ctx = new_ctx(b)
    assert ctx.n_obstacles == 9
    res = ctx.refine_allatom(chi)
    assert (out / "refine.csv").read_text() == refine_csv(protein["aaindex"], res.steps[:, 0].cpu().numpy(), (16, 8, 4), res.e[0].cpu().numpy(),
                                                            protein["chain_id"], protein["residue_index"])
    bare = new_ctx(protein_to_batch(protein)).refine_allatom(chi)
    assert not torch.equal(bare.e_round[0, ..., 0], res.e_round[0, ..., 0]), "the ligand atoms add terms"


def test_without_the_flag_eval_diffusion_writes_the_bytes_of_the_golden_run(tmp_path, capsys):
    """The golden run of tests/test_hip_cli.py (tests/golden/g21_cli_parent.txt: the SHA-256 of the structure.pdb an earlier commit
    wrote for exactly these arguments): unchanged without --refine_allatom, and the only file; with it structure.pdb changes and
    refine.csv appears.  mutate and proximal_optimize have no golden file in the suite: their runs are compared flag against no flag."""
    import hashlib
    import os
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.pdb_io import to_pdb
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    base = ["--input", str(pdb), "--molprobity_clash_loc", "/nonexistent", "--device", "cuda", "--random_weights", "3", "--steps", "10",
            "--seed", "5", "--use_proximal"]
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "plain")])
    assert sorted(os.listdir(tmp_path / "plain")) == ["structure.pdb"]
    golden = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g21_cli_parent.txt")).read().split()
    assert hashlib.sha256((tmp_path / "plain" / "structure.pdb").read_bytes()).hexdigest() == golden[0]
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "refined"), "--refine_allatom"])
    assert sorted(os.listdir(tmp_path / "refined")) == ["refine.csv", "structure.pdb"]
    assert (tmp_path / "refined" / "structure.pdb").read_bytes() != (tmp_path / "plain" / "structure.pdb").read_bytes()
    assert "all-atom refinement: energy " in capsys.readouterr().out
