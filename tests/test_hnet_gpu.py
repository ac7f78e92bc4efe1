"""Hydrogen-bond network optimisation on the device, through the C ABI (pp_hnet_optimize).

Reference: tests/hnet_oracle.py (brute force, no row filter, no partner cap, its own mover lists).  ``cand`` must lie within 1e-5 A +
2 ulp32(largest |coordinate|) of the float64 oracle (section 29's bound for ``hxyz``: the direction is built from differences to the
parent).  ``state``, ``e``, ``energy``, ``trace``, ``sweeps``, ``converged`` and ``hmask`` must have the BYTES of the float32 restatement
fed the device's own two coordinate sets and candidates (``hb``, the bond counts, too); ``xyz``, ``hxyz`` and ``chi`` the bytes of the selection.  Nothing measured on
the device enters a bound."""
import functools

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc

from . import allatom_oracle as A
from . import hnet_oracle as H
from . import polar_oracle as O
from .test_allatom_gpu import _pack3, _padded, arrays, hxyz_tolerance, new_ctx

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WORDS = ("state", "e", "hb", "energy", "trace", "sweeps", "converged")


def seeded_chi(b, seed=5):
    """Angles for a batch: its own where it has them for every row, with seeded noise on top so that flips and rotors have work."""
    g = torch.Generator().manual_seed(seed)
    chi = b["SC_D"].clone().float()
    return torch.remainder(chi + 0.5 * torch.randn(chi.shape, generator=g) + np.pi, 2 * np.pi) - np.pi


def host(t, *shape):
    return None if t is None else t.reshape(*shape).cpu().numpy()


def words(res):
    n = res.state.numel()
    return dict(state=host(res.state, n), e=host(res.e, n, 2), hb=host(res.hb, n, 2), energy=host(res.energy, n, 12), trace=host(res.trace, *res.trace.shape),
                sweeps=host(res.sweeps, -1), converged=host(res.converged, -1))


def problem(b, res, ctx=None, link=None, dtype=np.float32, cand=None, **kw):
    """The oracle's problem fed the DEVICE's own coordinate sets (and, unless ``cand`` is given, its candidates)."""
    _, am, rt, chain, offs = arrays(b)
    n = len(rt)
    x1 = res.xyz1 is not None
    return H.Problem(host(res.xyz0, n, 14, 3), host(res.hxyz0, n, 13, 3), host(res.hmask0, n, 13), rt, chain, offs, host(res.link_prev, n),
                     A.default_radius(rt, am, "keep"), rc.mover_extent, host(res.xyz1, n, 14, 3) if x1 else None,
                     host(res.hxyz1, n, 13, 3) if x1 else None, host(res.hmask1, n, 13) if x1 else None,
                     cand=host(res.cand, n, 12, 3, 3) if cand is None else cand, link=link, dtype=dtype, **kw)


def check_candidates(res, b, what=""):
    _, am, rt, chain, offs = arrays(b)
    n = len(rt)
    X = host(res.xyz0, n, 14, 3)
    want = H.candidates(X.astype(np.float64), rt, host(res.hmask0, n, 13), np.float64)
    got = host(res.cand, n, 12, 3, 3)
    err = float(np.abs(got - want).max())
    print(f"{what}: largest candidate error {err:.3g} A (bound {hxyz_tolerance(X):.3g})")
    assert np.isfinite(got).all() and err <= hxyz_tolerance(X), (what, err)
    # state 0 of a rotor is pp_hydrogens' placement, bit for bit
    h0 = host(res.hxyz0, n, 13, 3)
    for r in range(n):
        kind, ns, moved = H.mover_of_type(int(rt[r]))
        if kind == 1:
            for j, s in enumerate(moved):
                assert got[r, 0, j].tobytes() == h0[r, s - 14].tobytes(), (what, r, s)


def check_selection(res, b, ref_hmask, what=""):
    """xyz / hxyz / chi / hmask of the result are rows of the two sets, by ``state``."""
    _, am, rt, chain, offs = arrays(b)
    n = len(rt)
    st = host(res.state, n)
    flip = np.array([H.mover_of_type(int(t))[0] == 2 for t in rt]) & (st == 1)
    pick = lambda a0, a1, *sh: np.where(flip.reshape((n,) + (1,) * len(sh)), host(a1, n, *sh), host(a0, n, *sh)) if a1 is not None else host(a0, n, *sh)
    assert host(res.xyz, n, 14, 3).tobytes() == pick(res.xyz0, res.xyz1, 14, 3).tobytes(), what
    assert host(res.hmask, n, 13).tobytes() == ref_hmask.tobytes(), what
    assert host(res.hmask, n, 13).tobytes() == pick(res.hmask0, res.hmask1, 13).tobytes(), what
    want_h = pick(res.hxyz0, res.hxyz1, 13, 3).copy()
    cand, hm = host(res.cand, n, 12, 3, 3), host(res.hmask0, n, 13)
    for r in range(n):
        kind, ns, moved = H.mover_of_type(int(rt[r]))
        if kind == 1 and st[r] >= 0:
            for j, s in enumerate(moved):
                if hm[r, s - 14]:
                    want_h[r, s - 14] = cand[r, st[r], j]
    assert host(res.hxyz, n, 13, 3).tobytes() == want_h.tobytes(), what
    if res.chi is not None:
        assert host(res.chi, n, 4).tobytes() == pick(res.chi0, res.chi1, 4).tobytes(), what


def assert_same_words(got, want, what=""):
    for k in WORDS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        assert got[k].tobytes() == want[k].astype(np.int32).tobytes(), (what, k, int((got[k] != want[k]).sum()))


def run_and_check(b, chi, what, ctx=None, link=None, max_sweeps=32, ref_kw=None, **kw):
    """One call on the device against the oracle.  ``kw``: for both; ``ref_kw``: what only the oracle is told (the obstacle atoms)."""
    ctx = ctx or new_ctx(b)
    res = ctx.hbond_optimize(chi=None if chi is None else chi.to(DEV), link=link, max_sweeps=max_sweeps, want_candidates=True, **kw)
    check_candidates(res, b, what)
    lk = None if link is None else np.asarray(torch.as_tensor(link).cpu()).reshape(-1)
    ref = H.optimize(problem(b, res, ctx, link=lk, **kw, **(ref_kw or {})), max_sweeps)
    got = words(res)
    print(f"{what}: movers {int((got['state'] >= 0).sum())}, moved {int((got['state'] > 0).sum())}, trace {ref['trace'][:, 0].tolist()} -> "
          f"{ref['trace'][:, -1].tolist()}, sweeps {ref['sweeps'].tolist()}, words that differ {[int((got[k] != ref[k]).sum()) for k in WORDS]}")
    assert_same_words(got, ref, what)
    check_selection(res, b, ref["hmask_out"], what)
    offs = np.asarray(arrays(b)[4])
    assert np.array_equal(res.n_movers.cpu().numpy(), np.add.reduceat((got["state"] >= 0).astype(np.int64), offs[:-1]))
    assert ctx.saturated() == 0
    return ctx, res, ref


@functools.lru_cache(maxsize=None)
def solved(name):
    b = CASES[name]()
    return (b,) + run_and_check(b, seeded_chi(b), name)


SINGLES = ("c24", "c64", "c97", "1BRS", "2FTL", "damaged64")
CASES = {**{n: functools.partial(O.batch, n) for n in SINGLES}, "padded": _padded, "pack3": _pack3}


@pytest.mark.parametrize("name", sorted(CASES))
def test_words_against_the_oracle(name):
    b, ctx, res, ref = solved(name)
    st = ref["state"]
    assert (st > 0).sum() >= 1 and (ref["trace"][:, 0] > ref["trace"][:, -1]).all(), "vacuous: nothing moved"
    assert (np.diff(ref["trace"].astype(np.int64), axis=1) <= 0).all() and ref["converged"].all()
    # the angles of the result reconstruct to its heavy atoms, bit for bit
    assert torch.equal(ctx.atom14(res.chi), res.xyz.reshape(ctx.B, ctx.L, 14, 3))
    if name in ("c97", "1BRS", "2FTL"):
        kinds = {H.mover_of_type(int(t))[0] for t, s in zip(arrays(b)[2], st) if s > 0}
        assert kinds == {1, 2}, "a rotor and a flip moved"
    if name == "padded":
        assert (st[36 + 40:] == -1).all()


def test_rotors_alone_from_xyz_and_from_the_batch():
    b = O.batch("1BRS")
    ctx, res, ref = run_and_check(b, None, "1BRS, the batch's X")
    assert res.chi is None and res.xyz1 is None
    rt = arrays(b)[2]
    flips = np.array([H.mover_of_type(int(t))[0] == 2 for t in rt])
    assert (ref["state"][flips] == -1).all() and (ref["state"][~flips] > 0).sum() >= 1
    r2 = ctx.hbond_optimize(xyz=b["X"].to(DEV), want_candidates=True)
    assert_same_words(words(r2), words(res), "xyz= against the batch's X")


def test_the_same_words_alone_packed_as_a_decoy_and_twice():
    from packppi_amd.batch import replicate
    alone = {}
    for n in ("c97", "c65"):
        b = O.batch(n)
        chi = seeded_chi(b, 7)
        r = new_ctx(b).hbond_optimize(chi=chi.to(DEV), want_candidates=True)
        alone[n] = (words(r), host(r.hxyz, -1, 39), chi)
    b = _pack3()
    chi = torch.cat([alone[n][2].reshape(-1, 4) for n in ("c97", "c65", "c97")]).reshape(1, -1, 4)
    ctx = new_ctx(b)
    r1, r2 = ctx.hbond_optimize(chi=chi.to(DEV), want_candidates=True), ctx.hbond_optimize(chi=chi.to(DEV), want_candidates=True)
    assert_same_words(words(r1), words(r2), "two runs")
    assert torch.equal(r1.hxyz, r2.hxyz) and torch.equal(r1.xyz, r2.xyz)
    packed, hx = words(r1), host(r1.hxyz, -1, 39)
    for (lo, hi), n, s in (((0, 97), "c97", 0), ((97, 162), "c65", 1), ((162, 259), "c97", 2)):
        for k in ("state", "e", "hb", "energy"):
            assert packed[k][lo:hi].tobytes() == alone[n][0][k].tobytes(), (n, s, k)
        for k in ("trace", "sweeps", "converged"):
            assert packed[k][s].tobytes() == alone[n][0][k][0].tobytes(), (n, s, k)
        assert hx[lo:hi].tobytes() == alone[n][1].tobytes()
    bd = replicate(O.batch("c65"), 3)
    rd = new_ctx(bd).hbond_optimize(chi=torch.cat([alone["c65"][2].reshape(-1, 4)] * 3).reshape(1, -1, 4).to(DEV), want_candidates=True)
    dec = words(rd)
    for d in range(3):
        for k in ("state", "e", "hb", "energy"):
            assert dec[k][65 * d:65 * d + 65].tobytes() == alone["c65"][0][k].tobytes()
        assert dec["trace"][d].tobytes() == alone["c65"][0]["trace"][0].tobytes()


def test_three_decoys_at_three_chi_sets():
    from packppi_amd.batch import replicate
    b = replicate(O.batch("c24"), 3)
    g = torch.Generator().manual_seed(5)
    chi = (torch.rand(1, 72, 4, generator=g) * 2 - 1) * np.pi
    ctx, res, ref = run_and_check(b, chi, "three decoys")
    assert len({ref["energy"][24 * d:24 * d + 24].tobytes() for d in range(3)}) == 3


@pytest.mark.parametrize("rot_seed,shift", [(None, (1e4, -1e4, 1e4)), (1, (3.0, -7.0, 11.0)), (2, (1e4, 1e4, -1e4))])
def test_far_from_the_origin_and_under_a_rotation(rot_seed, shift):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(synth.rigid_motion(O.protein("c64"), rot_seed, np.array(shift)))
    run_and_check(b, seeded_chi(b), f"rotation {rot_seed}, shift {shift}")


@pytest.mark.parametrize("max_sweeps", [0, 1])
def test_few_sweeps(max_sweeps):
    b = O.batch("c64")
    ctx, res, ref = run_and_check(b, seeded_chi(b), f"max_sweeps {max_sweeps}", max_sweeps=max_sweeps)
    assert res.trace.shape == (1, max_sweeps + 1) and int(res.converged[0]) == 0 and int(res.sweeps[0]) == max_sweeps
    if max_sweeps == 0:
        st = host(res.state, -1)
        assert ((st == 0) | (st == -1)).all()
        assert torch.equal(res.hxyz.reshape(-1), res.hxyz0.reshape(-1)) and torch.equal(res.chi, res.chi0)
        # rotor state 0 and pp_hydrogens call one pp_nerf: the same words for every rotor hydrogen, and c64 is the smallest fixture
        # with a Ser, a Tyr and a Lys that have theirs
        n, rt = st.size, arrays(b)[2]
        cand, h0 = host(res.cand, n, 12, 3, 3).view(np.int32), host(res.hxyz0, n, 13, 3).view(np.int32)
        hm, seen = host(res.hmask0, n, 13), set()
        for r in range(n):
            kind, _, moved = H.mover_of_type(int(rt[r]))
            for j, s in enumerate(moved if kind == 1 else ()):
                if hm[r, s - 14]:
                    assert np.array_equal(cand[r, 0, j], h0[r, s - 14]), (r, s)
                    seen.add(rc.resnames[int(rt[r])])
        assert {"SER", "TYR", "LYS"} <= seen, seen


# ---- hand-built cases: obstacle atoms can be put anywhere --------------------------------------------------------------------------------
def row_of_type(rn, skip=0):
    """(fixture, row) of the (skip + 1)-th row of residue type ``rn`` with all its atoms, in the first fixture that has one."""
    t = rc.resname_to_idx[rn]
    for name in ("c97", "c64", "1BRS", "2FTL"):
        _, am, rt, _, _ = arrays(O.batch(name))
        rows = [r for r in range(len(rt)) if rt[r] == t and (am[r] != 0).sum() == int((rc.atom14_mask[t] != 0).sum())]
        if len(rows) > skip:
            return name, rows[skip]
    raise AssertionError(f"no fixture has a complete {rn}")


def only_rows(ctx, rows):
    """Radii that count the atoms of ``rows`` alone: whatever else the structure holds has no term."""
    r = torch.zeros_like(ctx.allatom_tables().radius)
    r[list(rows)] = ctx.allatom_tables().radius[list(rows)]
    return r.reshape(ctx.B, ctx.L, 27)


def only_moved(ctx, b, rows):
    """Radii that count the moved atoms of ``rows`` alone (the fixtures' own side chains overlap themselves in places)."""
    rt = arrays(b)[2]
    r = torch.zeros_like(ctx.allatom_tables().radius)
    for row in rows:
        moved = H.mover_of_type(int(rt[row]))[2]
        r[row, moved] = ctx.allatom_tables().radius[row, moved]
    return r.reshape(ctx.B, ctx.L, 27)


def beyond(h, d, length):
    """The point ``length`` A beyond h on the line from d through h (float64)."""
    u = (h - d) / np.linalg.norm(h - d)
    return h + length * u


@pytest.mark.parametrize("rn", sorted(H.ROTORS))
def test_a_polar_obstacle_beyond_a_state_makes_the_rotor_choose_it(rn):
    """For every state c: an acceptor 1.9 A beyond that state's (first) hydrogen on the line D -> h.  The limits are 2.0 A here: the
    hydrogens of the neighbouring states, 30 degrees on, are 2.06 A or more from that point (the chord of the hydrogen's circle is
    at least 2 x 0.905 x sin 15 degrees = 0.468 A, which puts them at sqrt(1.9^2 + 0.434 + 0.219) A), so only state c has a bond
    and no tie decides."""
    name, r = row_of_type(rn)
    b = O.batch(name)
    ctx = new_ctx(b)
    chi = b["SC_D"].float().to(DEV)
    rad = only_moved(ctx, b, [r])
    kw = dict(chi=chi, radius=rad, hb_weak=2.0, hb_good=2.0, want_candidates=True)
    free = ctx.hbond_optimize(**kw)
    n = free.state.numel()
    st, en, cand, xyz = host(free.state, n), host(free.energy, n, 12), host(free.cand, n, 12, 3, 3).astype(np.float64), host(free.xyz0, n, 14, 3)
    kind, ns, moved = H.mover_of_type(rc.resname_to_idx[rn])
    assert st[r] == 0 and (st[np.arange(n) != r] == -1).all(), "the one counted row is the one mover, and nothing pulls it"
    assert (en[r, :ns] == 0).all()
    parent = int(rc.hydrogen_parent[rc.resname_to_idx[rn], moved[0] - 14])
    for c in range(ns):
        spot = beyond(cand[r, c, 0], xyz[r, parent].astype(np.float64), 1.9)
        ctx.set_obstacles(torch.tensor([[*spot, 1.2]], dtype=torch.float32), polar=[1])
        res = ctx.hbond_optimize(**kw)
        e = host(res.energy, n, 12)[r]
        assert int(res.state.reshape(-1)[r]) == c, (rn, c, e[:ns].tolist())
        assert e[c] == en[r, c] - 2 and (np.delete(e[:ns], c) == np.delete(en[r, :ns], c)).all(), (rn, c, e[:ns].tolist())
        assert host(res.e, n, 2)[r].tolist() == [int(e[0]), int(e[c])] and int(res.sweeps[0]) == (1 if c else 0)
        assert host(res.hb, n, 2)[r].tolist() == [1 if c == 0 else 0, 1] and int(res.n_bonds[0]) == 1
        # not a polar atom: nothing to bond to, and 1.9 A is no overlap (1.0 + 1.2 - 0.4 = 1.8 A)
        ctx.set_obstacles(torch.tensor([[*spot, 1.2]], dtype=torch.float32), polar=[0])
        assert int(ctx.hbond_optimize(**kw).state.reshape(-1)[r]) == 0
    assert ctx.saturated() == 0


@pytest.mark.parametrize("rn", sorted(H.ROTORS))
def test_an_apolar_obstacle_on_state_0_makes_the_rotor_leave_it(rn):
    """A small sphere (0.1 A) a tenth of an angstrom beyond the conventional hydrogen: 1.0 + 0.1 - 0.4 = 0.7 A of allowed approach.
    State 0 overlaps it; a hydrogen 60 degrees on (a chord of 0.9 A or more) does not, and every rotor has a state whose nearest
    hydrogen is that far round -- a lysine only its state 2, whose three hydrogens sit at 60, 180 and 300 degrees from the spot."""
    name, r = row_of_type(rn)
    b = O.batch(name)
    ctx = new_ctx(b)
    chi = b["SC_D"].float().to(DEV)
    kw = dict(chi=chi, radius=only_moved(ctx, b, [r]), want_candidates=True)
    free = ctx.hbond_optimize(**kw)
    n = free.state.numel()
    kind, ns, moved = H.mover_of_type(rc.resname_to_idx[rn])
    parent = int(rc.hydrogen_parent[rc.resname_to_idx[rn], moved[0] - 14])
    spot = beyond(host(free.cand, n, 12, 3, 3)[r, 0, 0].astype(np.float64), host(free.xyz0, n, 14, 3)[r, parent].astype(np.float64), 0.1)
    ctx.set_obstacles(torch.tensor([[*spot, 0.1]], dtype=torch.float32))
    res = ctx.hbond_optimize(**kw)
    e = host(res.e, n, 2)[r]
    assert int(res.state.reshape(-1)[r]) > 0 and e[0] == host(free.e, n, 2)[r, 0] + 64 and e[1] <= e[0] - 64, (rn, e.tolist())
    assert int(res.converged[0]) == 1 and res.trace[0, 0] - res.trace[0, -1] >= 64


@pytest.mark.parametrize("rn", sorted(H.FLIPS))
def test_an_acceptor_only_the_flipped_hydrogens_reach_flips_the_row(rn):
    name, r = row_of_type(rn)
    b = O.batch(name)
    ctx = new_ctx(b)
    chi = b["SC_D"].float().to(DEV)
    kw = dict(chi=chi, radius=only_moved(ctx, b, [r]), want_candidates=True)
    free = ctx.hbond_optimize(**kw)
    n = free.state.numel()
    assert int(free.state.reshape(-1)[r]) == 0, "without the obstacle the row stays"
    t = rc.resname_to_idx[rn]
    kind, ns, moved = H.mover_of_type(t)
    hs = [s for s in moved if s >= 14 and rc.allatom_class[t, s] & rc.AA_POLAR_H][0]          # HD21 / HE21 / HE2
    parent = int(rc.hydrogen_parent[t, hs - 14])
    spot = beyond(host(free.hxyz1, n, 13, 3)[r, hs - 14].astype(np.float64), host(free.xyz1, n, 14, 3)[r, parent].astype(np.float64), 1.9)
    ctx.set_obstacles(torch.tensor([[*spot, 1.2]], dtype=torch.float32), polar=[1])
    res = ctx.hbond_optimize(**kw)
    e = host(res.energy, n, 12)[r]
    # state 1 gains the bond; state 0 has none (whatever the sphere touches there is an overlap, a multiple of 64)
    assert int(res.state.reshape(-1)[r]) == 1 and e[1] == host(free.energy, n, 12)[r, 1] - 2 and e[0] >= 0 and e[0] % 64 == 0, e[:2].tolist()
    assert torch.equal(res.xyz.reshape(-1, 14, 3)[r], res.xyz1.reshape(-1, 14, 3)[r]) and torch.equal(res.chi.reshape(-1, 4)[r], res.chi1.reshape(-1, 4)[r])
    assert not torch.equal(res.chi.reshape(-1, 4)[r], res.chi0.reshape(-1, 4)[r])
    assert torch.equal(ctx.atom14(res.chi), res.xyz.reshape(ctx.B, ctx.L, 14, 3))
    ctx.set_obstacles(None)
    assert int(ctx.hbond_optimize(**kw).state.reshape(-1)[r]) == 0


def test_two_coupled_movers_move_one_per_sweep():
    """Two serines or threonines 8 to 10.5 A apart (partners: 3.9 + 3.9 + 3.2 A; too far for a term between them), each with an
    acceptor beyond its state 6: equal gains, so the lower row moves in sweep 1 and the higher in sweep 2."""
    b = O.batch("2FTL")
    X, am, rt, chain, offs = arrays(b)
    rot = [r for r in range(len(rt)) if rc.resnames[rt[r]] in ("SER", "THR") and (am[r, :7] != 0).all()]
    pair = next((i, j) for i in rot for j in rot if i < j and 8.0 <= np.linalg.norm(X[i, 1] - X[j, 1]) <= 10.5)
    ctx = new_ctx(b)
    kw = dict(chi=b["SC_D"].float().to(DEV), radius=only_rows(ctx, pair), hb_weak=2.0, hb_good=2.0, want_candidates=True)
    free = ctx.hbond_optimize(**kw)
    n = free.state.numel()
    cand, xyz = host(free.cand, n, 12, 3, 3).astype(np.float64), host(free.xyz0, n, 14, 3).astype(np.float64)
    spots = []
    for r in pair:
        t = int(rt[r])
        parent = int(rc.hydrogen_parent[t, H.mover_of_type(t)[2][0] - 14])
        spots.append([*beyond(cand[r, 6, 0], xyz[r, parent], 1.9), 1.4])
    ctx.set_obstacles(torch.tensor(spots, dtype=torch.float32), polar=[1, 1])
    one = ctx.hbond_optimize(max_sweeps=1, **kw)
    assert host(one.state, n)[list(pair)].tolist() == [6, 0] and int(one.converged[0]) == 0
    res = ctx.hbond_optimize(**kw)
    assert host(res.state, n)[list(pair)].tolist() == [6, 6] and int(res.sweeps[0]) == 2 and int(res.converged[0]) == 1
    tr = host(res.trace, 1, 33)[0]
    assert tr[0] - tr[1] == 2 and tr[1] - tr[2] == 2 and (tr[2:] == tr[2]).all()


def test_obstacles_against_the_oracle():
    """1BRS with 40 obstacle atoms put next to its movers, half of them polar: the words of the float32 restatement."""
    b = O.batch("1BRS")
    ctx = new_ctx(b)
    chi = seeded_chi(b)
    free = ctx.hbond_optimize(chi=chi.to(DEV), want_candidates=True)
    n = free.state.numel()
    rows = np.nonzero(host(free.state, n) >= 0)[0][:40]
    rng = np.random.default_rng(3)
    xyz = host(free.xyz0, n, 14, 3)
    spots = np.concatenate([xyz[rows, 5] + rng.normal(size=(40, 3)) * 2.0, np.full((40, 1), 1.5)], 1).astype(np.float32)
    polar = (np.arange(40) % 2).astype(np.uint8)
    ctx.set_obstacles(torch.from_numpy(spots), polar=polar)
    _, res, ref = run_and_check(b, chi, "1BRS with obstacles", ctx=ctx, ref_kw=dict(obst=spots, obst_off=[0, 40], obst_polar=polar))
    assert not np.array_equal(host(res.e, n, 2), host(free.e, n, 2))
    # obst_polar of the call overrides the context's
    none = ctx.hbond_optimize(chi=chi.to(DEV), obst_polar=np.zeros(40, np.uint8), want_candidates=True)
    ref0 = H.optimize(problem(b, none, obst=spots, obst_off=[0, 40], obst_polar=np.zeros(40, np.uint8)), 32)
    assert_same_words(words(none), ref0, "no polar obstacle")
    assert not np.array_equal(ref0["e"], ref["e"])


def test_a_row_over_the_partner_list_capacity_gets_the_words_of_the_oracle():
    """dense_complex() of tests/test_clash_capacity.py: 126 movers have more than PP_HNET_PCAP partners (up to 125) and scan, 33 have
    fewer and read their list; the oracle has no list."""
    from .test_clash_capacity import dense_complex
    b = dense_complex()
    ctx, res, ref = run_and_check(b, b["SC_D"].float(), "dense", max_sweeps=3)
    n_partners = np.array([len(ref["plist"][r]) for r in sorted(ref["plist"])])
    assert (n_partners > 16).sum() >= 100 and (n_partners <= 16).sum() >= 20 and ref["sweeps"][0] == 3


def test_a_bonded_cysteine_is_no_mover():
    name = next(nm for nm in ("2FTL", "1BRS", "c97", "c64") if (arrays(O.batch(nm))[2] == rc.resname_to_idx["CYS"]).sum() >= 2)
    b = O.batch(name)
    rt = arrays(b)[2]
    i, j = np.nonzero(rt == rc.resname_to_idx["CYS"])[0][:2]
    link = -np.ones(len(rt), np.int32)
    link[i], link[j] = j, i
    chi = seeded_chi(b)
    ctx, res, ref = run_and_check(b, chi, f"{name} with a disulfide", link=torch.from_numpy(link))
    st = host(res.state, -1)
    assert st[i] == -1 and st[j] == -1 and (host(res.hmask, -1, 13)[[i, j], 4] == 0).all()
    free = host(ctx.hbond_optimize(chi=chi.to(DEV)).state, -1)
    assert free[i] >= 0 and free[j] >= 0


def test_a_bad_table_entry_is_found_on_the_device():
    b = O.batch("c97")
    rt = arrays(b)[2]
    chi = seeded_chi(b).to(DEV)
    ser = rc.resname_to_idx["SER"]
    assert (rt == ser).sum() >= 1
    good = host(new_ctx(b).hbond_optimize(chi=chi).state, -1)
    for col, val in ((0, 3), (0, -1), (1, 13), (1, 0), (2, 1 << 27), (2, 1 << 3), (2, 0)):
        tab = rc.mover_table.copy()
        tab[ser, col] = val
        ctx = new_ctx(b)
        st = host(ctx.hbond_optimize(chi=chi, mover=tab).state, -1)
        assert (st[rt == ser] == -1).all() and (st[rt != ser] >= 0).sum() == (good[rt != ser] >= 0).sum(), (col, val)
        assert ctx.saturated() == 8, (col, val)
    tab = rc.mover_table.copy()
    tab[rc.resname_to_idx["ASN"], 1] = 3                       # a flip has two states
    ctx = new_ctx(b)
    st = host(ctx.hbond_optimize(chi=chi, mover=tab).state, -1)
    assert (st[rt == rc.resname_to_idx["ASN"]] == -1).all() and ctx.saturated() == 8


def test_refusals():
    from packppi_amd import lib as L
    b = O.batch("c24")
    ctx = new_ctx(b)
    chi = b["SC_D"].float().to(DEV)
    for kw, msg in ((dict(max_sweeps=-1), "max_sweeps"), (dict(max_sweeps=257), "max_sweeps"), (dict(hb_weak=float("nan")), "finite"),
                    (dict(cut=float("inf")), "finite"), (dict(hb_allow=-0.1), "hb_allow"), (dict(hb_good=3.0), "hb_good"),
                    (dict(hb_good=0.0), "hb_good"), (dict(obst_polar=[1]), "obstacle"), (dict(mover=np.zeros((20, 4))), "mover"),
                    (dict(radius=torch.zeros(5)), "radius")):
        with pytest.raises(ValueError, match=msg):
            ctx.hbond_optimize(chi=chi, **kw)
    with pytest.raises(ValueError, match="link"):
        ctx.hbond_optimize(chi=chi, link=np.zeros(3, np.int32))
    # the C entry itself
    res = ctx.hbond_optimize(chi=chi, want_candidates=True)
    tabs, ht = ctx.allatom_tables(), ctx.hnet_tables()
    lib, ptr = L.load(), L._ptr
    f32 = np.float32

    def call(**over):
        a = dict(xyz0=res.xyz0, hxyz0=res.hxyz0, hmask0=res.hmask0, xyz1=res.xyz1, hxyz1=res.hxyz1, hmask1=res.hmask1, chi0=res.chi0,
                 chi1=res.chi1, place=tabs.place, param=tabs.param, mover=ht.mover, rot=ht.rot, ext=ht.ext, radius=tabs.radius,
                 acls=tabs.acls, aa_sep=tabs.aa_sep, link_prev=res.link_prev, link=None, obst_polar=None, cut=0.4, hb_allow=0.6,
                 hb_weak=2.5, hb_weak2=float(f32(2.5) * f32(2.5)), hb_good2=float(f32(2.2) * f32(2.2)), reach=3.2, max_sweeps=4,
                 state=torch.empty_like(res.state), xyz_out=torch.empty_like(res.xyz), hxyz_out=torch.empty_like(res.hxyz),
                 hmask_out=torch.empty_like(res.hmask), chi_out=torch.empty_like(res.chi), e=torch.empty_like(res.e), hb=None,
                 trace=torch.empty(1, 5, dtype=torch.int32, device=DEV), sweeps=torch.empty_like(res.sweeps),
                 converged=torch.empty_like(res.converged), cand=None, energy=None)
        a.update(over)
        args = [ptr(v) if (isinstance(v, torch.Tensor) or v is None) else v for v in a.values()]
        return lib.pp_hnet_optimize(ctx.handle, *args, ctx._stream()), a

    rc_, a = call()
    assert rc_ == 0 and torch.equal(a["state"], ctx.hbond_optimize(chi=chi, max_sweeps=4).state)
    for k in ("xyz0", "hxyz0", "hmask0", "place", "param", "mover", "rot", "ext", "radius", "acls", "aa_sep", "link_prev", "state",
              "xyz_out", "hxyz_out", "hmask_out", "e", "trace", "sweeps", "converged"):
        assert call(**{k: None})[0] == 1 and b"pp_hnet_optimize" in lib.pp_last_error(), k
    for over in (dict(xyz1=None), dict(hxyz1=None), dict(hmask1=None), dict(chi0=None), dict(chi1=None), dict(chi_out=None),
                 dict(xyz1=None, hxyz1=None, hmask1=None), dict(cut=float("nan")), dict(hb_allow=-1.0), dict(hb_allow=float("inf")),
                 dict(hb_weak=0.0), dict(hb_weak2=float("nan")), dict(hb_good2=-1.0), dict(hb_good2=7.0), dict(reach=float("inf")),
                 dict(reach=1.0), dict(max_sweeps=-1), dict(max_sweeps=257), dict(obst_polar=res.hmask0)):
        assert call(**over)[0] == 1 and b"pp_hnet_optimize" in lib.pp_last_error(), over
    assert lib.pp_hnet_optimize(None, *[None] * 19, 0.4, 0.6, 2.5, 6.25, 4.84, 3.2, 4, *[None] * 13) == 1
    # rotors alone: no second set, no angles
    assert call(xyz1=None, hxyz1=None, hmask1=None, chi0=None, chi1=None, chi_out=None)[0] == 0
    assert ctx.saturated() == 0


@pytest.mark.parametrize("name", SINGLES)
def test_the_optimised_hydrogens_do_not_overlap_more(name):
    """``clashscore`` takes the result as its ``hydrogens``; with the rotatable hydrogens counted, the serious overlaps that involve
    one are no more than at the conventional placement."""
    b, ctx, res, ref = solved(name)
    chi = seeded_chi(b).to(DEV)
    rot = ctx.allatom_tables().rotatable.reshape(-1, 27)
    before = ctx.clashscore(chi=chi, rotatable="keep")
    after = ctx.clashscore(chi=res.chi, hydrogens=res, rotatable="keep")
    count = lambda r: int(r.n_clash.reshape(-1, 27, 2).sum(-1)[rot].sum())
    print(f"{name}: overlaps with a rotatable hydrogen {count(before)} -> {count(after)}; clashscore {float(before.clashscore[0]):.2f} -> "
          f"{float(after.clashscore[0]):.2f}")
    assert torch.equal(after.hxyz, res.hxyz) and torch.equal(after.xyz.reshape(-1), res.xyz.reshape(-1))
    assert count(after) <= count(before)


# ---- the surfaces --------------------------------------------------------------------------------------------------------------------------
def test_functional_entry_and_the_ensemble_columns(weights):
    from packppi_amd.functional import optimize_hydrogens
    from packppi_amd.module import TDiffusionModule
    b = O.batch("c24")
    chi = seeded_chi(b).to(DEV)
    a, c = optimize_hydrogens(b.to(DEV), chi, want_candidates=True), new_ctx(b).hbond_optimize(chi=chi, want_candidates=True)
    assert_same_words(words(a), words(c), "functional")
    assert torch.equal(a.hxyz, c.hxyz) and torch.equal(a.chi, c.chi)
    assert optimize_hydrogens(b.to(DEV)).chi is None
    model = TDiffusionModule(weights, device=DEV)
    model.schedule = torch.linspace(1, 0, 4)
    gb = O.batch("c64").to(DEV)
    plain = model.sample_ensemble(gb, 3, seed=11, return_all=True, clashscore=True)
    out = model.sample_ensemble(gb, 3, seed=11, return_all=True, clashscore=True, hbond_optimize=True)
    assert set(out) - set(plain) == {"hnet_bonds", "hnet_flips", "clashscore_hnet"}
    for k in plain:
        if isinstance(plain[k], torch.Tensor):
            assert torch.equal(plain[k], out[k]), k
    dchi, packed = out["decoys"]
    ctx = new_ctx(packed)
    res = ctx.hbond_optimize(chi=dchi)
    assert out["hnet_bonds"].shape == (3,) and torch.equal(out["hnet_bonds"], res.n_bonds) and torch.equal(out["hnet_flips"], res.n_flips)
    assert torch.equal(res.n_bonds, res.hb.reshape(-1, 2)[:, 1].reshape(3, -1).sum(1)) and int(res.n_bonds.sum()) > 0
    want = ctx.clashscore(chi=res.chi, hydrogens=res, rotatable="keep").clashscore
    assert torch.equal(out["clashscore_hnet"], want) and not torch.equal(want, out["clashscore"])
    only = model.sample_ensemble(gb, 3, seed=11, return_all=True, hbond_optimize=True)
    assert "clashscore_hnet" not in only and torch.equal(only["hnet_flips"], out["hnet_flips"])
    assert torch.equal(model.sample_ensemble(gb, 3, seed=11, hbond_optimize=True), model.sample_ensemble(gb, 3, seed=11))


def _files(plain, flagged, extra):
    """``flagged`` holds every file of ``plain`` and exactly the ``extra`` names more; returns the common files whose bytes differ."""
    a, b = {p.name for p in plain.iterdir()}, {p.name for p in flagged.iterdir()}
    assert b - a == set(extra) and a <= b, (sorted(a), sorted(b))
    return [n for n in sorted(a) if (plain / n).read_bytes() != (flagged / n).read_bytes()]


def test_eval_diffusion_with_and_without_hnet(tmp_path, capsys):
    from packppi_amd import synth
    from packppi_amd.analysis import HNET_CSV_HEADER, hnet_csv
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    src = str(tmp_path / "in.pdb")
    with open(src, "w") as fh:
        fh.write(to_pdb(synth.make_complex(64, 11)))
    base = ["--input", src, "--molprobity_clash_loc", "none", "--random_weights", "0", "--seed", "7", "--steps", "3", "--device", DEV]
    plain, both, flagged = tmp_path / "plain", tmp_path / "both", tmp_path / "flagged"
    eval_diffusion.main(base + ["--outdir", str(plain)])
    eval_diffusion.main(base + ["--outdir", str(both), "--clashscore", "--hydrogens"])
    assert "hydrogen-bond network" not in capsys.readouterr().out
    eval_diffusion.main(base + ["--outdir", str(flagged), "--clashscore", "--hydrogens", "--hnet"])
    text = capsys.readouterr().out
    assert set(_files(both, flagged, ["hnet.csv"])) <= {"structure.pdb", "structure_H.pdb", "clashes.csv"}
    assert set(_files(plain, flagged, ["hnet.csv", "clashes.csv", "structure_H.pdb"])) <= {"structure.pdb"}
    protein = from_pdb_file(src)
    b = protein_to_batch(protein).to(DEV)
    args = eval_diffusion.parse_args(base + ["--outdir", str(tmp_path / "again")])
    chi = eval_diffusion.load_model(args).sampling(b, seed=7)
    ctx = new_ctx(b)
    res = ctx.hbond_optimize(chi=chi)
    got = (flagged / "hnet.csv").read_text()
    assert got == hnet_csv(protein["aaindex"], res.state[0].cpu().numpy(), res.e[0].cpu().numpy(), protein["chain_id"], protein["residue_index"])
    assert got.startswith(HNET_CSV_HEADER + "\n") and ",flip,1,180.0," in got and ",rotor," in got
    tr = res.trace[0].tolist()
    assert f"hydrogen-bond network: {int(res.n_movers[0])} movers, energy {tr[0]} -> {tr[-1]} in {int(res.sweeps[0])} sweeps -----" in text
    conv, opt = ctx.clashscore(chi=chi, rotatable="keep"), ctx.clashscore(chi=res.chi, hydrogens=res, rotatable="keep")
    assert (f"clashscore with the rotatable hydrogens counted: {float(conv.clashscore[0]):.2f} as placed, "
            f"{float(opt.clashscore[0]):.2f} with the hydrogen-bond network optimised (--hnet)") in text
    # structure.pdb holds the flips; structure_H.pdb its heavy atoms bit for bit and the optimised hydrogens
    a, c = from_pdb_file(flagged / "structure_H.pdb"), from_pdb_file(flagged / "structure.pdb")
    assert all(a[k].tobytes() == c[k].tobytes() for k in c)
    want_xyz = np.round(res.xyz[0].cpu().numpy().astype(np.float64), 3)
    m = c["atom_mask"] != 0
    assert np.abs(c["atom_positions"][m] - want_xyz[:len(m)][m]).max() <= 1.5e-3
    assert (flagged / "structure.pdb").read_bytes() != (plain / "structure.pdb").read_bytes()
    hs = {(ln[21], int(ln[22:26]), ln[12:16].strip()): [float(ln[30:38]), float(ln[38:46]), float(ln[46:54])]
          for ln in (flagged / "structure_H.pdb").read_text().splitlines() if ln.startswith("ATOM") and ln[76:78].strip() == "H"}
    assert len(hs) == int(res.hmask.sum())
    # decoys: ensemble.csv gains the columns, hnet.csv appears, every other file is as without the flag
    e0, e1 = tmp_path / "ens0", tmp_path / "ens1"
    eval_diffusion.main(base + ["--outdir", str(e0), "--n_decoys", "2"])
    eval_diffusion.main(base + ["--outdir", str(e1), "--n_decoys", "2", "--hnet"])
    assert _files(e0, e1, ["hnet.csv"]) == ["ensemble.csv"]
    r0 = [ln.split(",") for ln in (e0 / "ensemble.csv").read_text().strip().split("\n")]
    r1 = [ln.split(",") for ln in (e1 / "ensemble.csv").read_text().strip().split("\n")]
    assert r1[0] == r0[0] + ["hnet_bonds", "hnet_flips"] and [r[:-2] for r in r1] == r0 and len(r1) == 3
    assert all(int(r[-2]) >= 0 and int(r[-1]) >= 0 for r in r1[1:])


def test_mutate_and_proximal_optimize_with_and_without_hnet(tmp_path, capsys):
    from packppi_amd.analysis import HNET_CSV_HEADER
    from packppi_amd.cli import mutate, proximal_optimize
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    pdb = tmp_path / "1brs.pdb"
    pdb.write_text(to_pdb(O.protein("1BRS")))
    base = ["--input", str(pdb), "--mutstr", "LA87F", "--device", "cuda", "--random_weights", "3", "--steps", "3", "--seed", "7",
            "--n_decoys", "2"]
    m0, m1 = tmp_path / "m0", tmp_path / "m1"
    mutate.main(base + ["--outdir", str(m0), "--hydrogens"])
    mutate.main(base + ["--outdir", str(m1), "--hydrogens", "--hnet"])
    assert set(_files(m0, m1, ["hnet_LA87F.csv"])) <= {"mutants.csv", "mutant_LA87F.pdb", "mutant_LA87F_H.pdb"}
    r0 = [ln.split(",") for ln in (m0 / "mutants.csv").read_text().splitlines()]
    r1 = [ln.split(",") for ln in (m1 / "mutants.csv").read_text().splitlines()]
    assert r1[0] == r0[0] + ["hnet_bonds", "hnet_flips"] and [r[:-2] for r in r1] == r0 and int(r1[1][-2]) > 0
    assert (m1 / "hnet_LA87F.csv").read_text().startswith(HNET_CSV_HEADER + "\n")
    a, c = from_pdb_file(m1 / "mutant_LA87F_H.pdb"), from_pdb_file(m1 / "mutant_LA87F.pdb")
    assert all(a[k].tobytes() == c[k].tobytes() for k in c)
    assert (m1 / "mutant_LA87F_H.pdb").read_bytes() != (m0 / "mutant_LA87F_H.pdb").read_bytes()
    capsys.readouterr()
    pbase = ["--input", str(pdb), "--molprobity_clash_loc", "none", "--num_steps", "5", "--device", "cuda"]
    p0, p1 = tmp_path / "p0", tmp_path / "p1"
    proximal_optimize.main(pbase + ["--outdir", str(p0), "--clashscore", "--hydrogens"])
    assert "hydrogen-bond network" not in capsys.readouterr().out
    proximal_optimize.main(pbase + ["--outdir", str(p1), "--clashscore", "--hydrogens", "--hnet"])
    out = capsys.readouterr().out
    assert "hydrogen-bond network: " in out and "clashscore with the rotatable hydrogens counted: " in out
    assert set(_files(p0, p1, ["hnet.csv"])) <= {"structure.pdb", "structure_H.pdb", "clashes.csv"}
    assert (p1 / "structure_H.pdb").read_bytes() != (p0 / "structure_H.pdb").read_bytes()
    a, c = from_pdb_file(p1 / "structure_H.pdb"), from_pdb_file(p1 / "structure.pdb")
    assert all(a[k].tobytes() == c[k].tobytes() for k in c)
