"""CPU: the mover tables, the oracle and the text of the hydrogen-bond network optimisation.

The tables of ``packppi_amd.constants`` are derived (rotatable hydrogens, the rigid group of the flipped chi); here they are held
against the oracle's literal lists.  The oracle (tests/hnet_oracle.py) is held against the definition: F against a direct double loop
over atom pairs written with scalars, the descent's integers, and float32 against float64."""
import functools

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc

from . import allatom_oracle as A
from . import hnet_oracle as H
from . import polar_oracle as O

FIXTURES = ("c24", "c64", "c97", "1BRS", "2FTL")


# ---- the tables --------------------------------------------------------------------------------------------------------------------------
def test_which_types_have_movers_and_what_moves():
    kinds = {rc.resnames[t]: int(rc.mover_table[t, 0]) for t in range(21)}
    assert {n for n, k in kinds.items() if k == rc.MOVER_ROTOR} == {"SER", "THR", "CYS", "TYR", "LYS"} == set(H.ROTORS)
    assert {n for n, k in kinds.items() if k == rc.MOVER_FLIP} == {"ASN", "GLN", "HIS"} == set(H.FLIPS)
    assert rc.mover_table.shape == (21, 4) and rc.mover_table.dtype == np.int32 and (rc.mover_table[:, 3] == 0).all()
    for t, rn in enumerate(rc.resnames):
        kind, ns, moved = H.mover_of_type(t)
        assert (int(rc.mover_table[t, 0]), int(rc.mover_table[t, 1])) == (kind, ns), rn
        assert [s for s in range(27) if int(rc.mover_table[t, 2]) >> s & 1] == moved, rn
        want = list(H.ROTORS[rn][0]) if rn in H.ROTORS else list(H.FLIPS[rn][1]) if rn in H.FLIPS else []
        assert sorted(rc.mover_moved_names(t)) == sorted(want), rn
        assert len(moved) <= rc.PP_HNET_MOVED and ns <= rc.PP_HNET_STATES
    assert {rn: ns for rn, (_, ns) in ((r, (0, len(v[1]))) for r, v in H.ROTORS.items())} == dict(SER=12, THR=12, CYS=12, TYR=2, LYS=4)
    assert rc.mover_flip_chi == {rn: v[0] for rn, v in H.FLIPS.items()}


def test_rotor_states():
    for t, rn in enumerate(rc.resnames):
        if rn not in H.ROTORS:
            assert (rc.mover_rotor_cs[t] == 0).all()
            continue
        names, degs = H.ROTORS[rn]
        hyd = [rc.hydrogen_names[t].index(n) for n in names]
        for j, k in enumerate(hyd):
            # state 0: the very values of the placement, not a recomputation of them
            assert rc.mover_rotor_cs[t, 0, j].tobytes() == rc.hydrogen_param[t, k, 3:5].tobytes(), (rn, j)
            assert int(rc.hydrogen_place[t, k, 0]) & 15 == rc.H_NERF
            for c, deg in enumerate(degs):
                a = np.deg2rad(deg + 120.0 * j)
                assert np.allclose(rc.mover_rotor_cs[t, c, j], [np.cos(a), np.sin(a)], atol=1e-6), (rn, c, j)
                assert rc.mover_state_angle(t, c) == deg % 360.0
        assert (rc.mover_rotor_cs[t, len(degs):] == 0).all() and (rc.mover_rotor_cs[t, :, len(hyd):] == 0).all()
    assert rc.mover_state_angle(rc.resname_to_idx["ASN"], 1) == 180.0


def test_ext_bounds_the_farthest_moved_atom_over_a_chi_grid():
    """Every type with a mover, chi on a grid of 60 degrees (all four angles), both flip states and every rotor state: no moved atom
    is farther from CA than ``mover_extent``."""
    from oracle import ref_cpu as R
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(synth.make_complex(24, 5))
    X, bb = b["X"].double()[:, :1], b["BB_D"].double()[:, :1]
    grid = np.deg2rad(np.arange(-180.0, 180.0, 60.0))
    chis = np.stack(np.meshgrid(grid, grid, grid, grid, indexing="ij"), -1).reshape(-1, 4)
    seen = 0
    for t in range(20):
        kind, ns, moved = H.mover_of_type(t)
        if not kind:
            assert rc.mover_extent[t] == 0
            continue
        n = len(chis)
        rt = torch.full((1, n), t, dtype=torch.long)
        xyz = R.atom14_coords(X.expand(1, n, 14, 3), rt, bb.expand(1, n, 3), torch.from_numpy(chis)[None]).reshape(n, 14, 3).numpy()
        am = np.asarray(rc.atom14_mask[t] != 0, np.float32)[None].repeat(n, 0)
        h, m, _ = A.hydrogens(xyz, am, rt.reshape(-1).numpy(), np.zeros(n, np.int64), list(range(n + 1)))
        far = 0.0
        heavy, hyd = [s for s in moved if s < 14], [s - 14 for s in moved if s >= 14]
        if heavy:
            far = max(far, np.linalg.norm(xyz[:, heavy] - xyz[:, 1:2], axis=-1).max())
        if kind == 2:
            far = max(far, np.linalg.norm(h[:, hyd] - xyz[:, 1:2], axis=-1).max())
        else:
            cand = H.candidates(xyz, rt.reshape(-1).numpy(), m)
            far = max(far, np.linalg.norm(cand[:, :ns, :len(hyd)] - xyz[:, None, None, 1], axis=-1).max())
        assert m[:, hyd].all()
        print(f"{rc.resnames[t]}: farthest moved atom {far:.3f} A, ext {rc.mover_extent[t]:.3f} A")
        assert 2.0 < far <= rc.mover_extent[t], rc.resnames[t]
        seen += 1
    assert seen == 8


# ---- the oracle against the definition ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def descent(name, dtype=np.float64, accept="rule"):
    p = H.host_problem(O.batch(name), dtype=dtype)
    start = H.host_problem(O.batch(name), dtype=dtype)
    return start, p, H.optimize(p, 32, accept)


def _sep(p, i, x, j, y):
    if i == j:
        return int(p.sep[i][x, y])
    best = 99
    same = p.seg_of[i] == p.seg_of[j]
    if same and j == i + 1 and p.link_prev[j]:
        best = min(best, int(p.sep[i][x, 2]) + 1 + int(p.sep[j][0, y]))
    if same and j == i - 1 and p.link_prev[i]:
        best = min(best, int(p.sep[i][x, 0]) + 1 + int(p.sep[j][2, y]))
    return best


def direct_F(p):
    """F by the definition, scalar by scalar: every pair of counted atoms of a segment of which at least one is a moved atom of a
    mover and which are not moved atoms of the same mover, once.  Pairs farther apart than 4 A (no radius sum, no bond reaches
    that far) are left out before the scalar loop."""
    tot = np.zeros(len(p.seg_off) - 1, np.int64)
    cut, hba, hbw2, hbg2 = float(p.cut), float(p.hb_allow), float(p.hbw2), float(p.hbg2)
    for n in p.movers:
        s = int(p.seg_of[n])
        lo, hi = p.seg_off[s], p.seg_off[s + 1]
        for x in p.moved[n]:
            if not p.cur_w[n, x] > 0:
                continue
            px = p.cur[n, x].astype(np.float64)
            d = np.linalg.norm(p.cur[lo:hi].astype(np.float64) - px, axis=-1)
            for jr, y in zip(*np.nonzero((d <= 4.0) & (p.cur_w[lo:hi] > 0))):
                j = lo + int(jr)
                if j == n and y in p.moved[n]:
                    continue
                if p.is_moved[j, y] and (j, y) < (n, x):
                    continue                                    # counted from the other end
                xi, yi = int(p.cls[n, x]), int(p.cls[j, y])
                if _sep(p, n, x, j, int(y)) <= (4 if (xi | yi) & 4 else 3):
                    continue
                q = p.cur[j, y].astype(np.float64)
                dist2 = float(((q - px) ** 2).sum())
                xh, yh = bool(xi & 1 and yi & 2), bool(xi & 2 and yi & 1)
                t = float(p.cur_w[n, x]) + float(p.cur_w[j, y]) - cut - (hba if xh or yh else 0.0)
                term = 64 if (t > 0 and dist2 <= t * t) else 0
                if (xh or yh) and j != n:
                    hrow, hs, acc = (n, x, q) if xh else (j, int(y), px)
                    hpos = p.cur[hrow, hs].astype(np.float64)
                    par = p.cur[hrow, p.parent[hrow, hs]].astype(np.float64)
                    v, w = acc - hpos, par - hpos
                    sdot = float(v @ w)
                    if dist2 <= hbw2 and sdot <= 0:
                        good = dist2 <= hbg2 and sdot * sdot >= 0.25 * float(w @ w) * dist2
                        term -= 2 if good else 1
                tot[s] += term
    return tot


@pytest.mark.parametrize("name", FIXTURES)
def test_F_equals_a_direct_double_loop(name):
    start, p, r = descent(name)
    assert np.array_equal(start.F(), direct_F(start)) and np.array_equal(start.F(), r["trace"][:, 0])
    assert np.array_equal(p.F(), direct_F(p)) and np.array_equal(p.F(), r["trace"][:, -1])
    assert abs(int(start.F()[0])) > 0


@pytest.mark.parametrize("name", FIXTURES)
def test_the_descent_is_monotone_in_integers_and_ends_in_a_local_optimum(name):
    start, p, r = descent(name)
    tr, k = r["trace"][0].astype(np.int64), int(r["sweeps"][0])
    assert k >= 1 and r["converged"][0] == 1 and len(r["history"][k:]) == 32 - k and not any(r["history"][k:])
    assert (np.diff(tr[:k + 1]) < 0).all() and (tr[k:] == tr[k]).all()
    for q in range(k):
        acc = r["history"][q]
        assert acc and all(g > 0 for _, _, _, g in acc)
        assert tr[q] - tr[q + 1] == sum(g for _, _, _, g in acc), (name, q)
        rows = [n for n, _, _, _ in acc]
        assert not any(m in r["plist"][n] for n in rows for m in rows), "two accepted movers are partners"
    # P is symmetric, and holds every pair of movers with a term in the start state
    for n in p.movers:
        assert all(n in r["plist"][m] for m in r["plist"][n])
    # a local optimum: no single mover gains by any other state
    for n in p.movers:
        e = [p.energy(n, c) for c in range(int(p.ns[n]))]
        assert min(e) == e[int(p.state[n])], (name, n)
    assert (r["e"][p.movers, 1] <= r["e"][p.movers, 0]).sum() >= 1


def test_partners_hold_every_pair_of_movers_with_a_term():
    """Over all states of both: movers whose moved atoms come within reach of each other are partners (1BRS and c97)."""
    for name in ("1BRS", "c97"):
        start, _, r = descent(name)
        reach = float(start.reach)
        pos = {n: np.concatenate([start.atoms_at(n, c)[0] for c in range(int(start.ns[n]))]) for n in start.movers}
        pairs = 0
        for n in start.movers:
            for m in start.movers:
                if m > n and np.linalg.norm(pos[n][:, None] - pos[m][None], axis=-1).min() <= reach:
                    assert m in r["plist"][n], (name, n, m)
                    pairs += 1
        assert pairs >= 1, "vacuous: no two movers come within reach"


def test_accepting_every_positive_proposal_at_once():
    """Without the partner rule the drop of F is not the sum of the gains: two neighbours that both move change the term between
    them twice.  On these five inputs F still never rises; the inequality is what the rule buys, recorded here."""
    differs = 0
    for name in FIXTURES:
        _, _, r = descent(name, accept="all")
        tr = r["trace"][0].astype(np.int64)
        assert (np.diff(tr) <= 0).all(), name                  # monotone on all five: no counterexample among them to show
        for q, acc in enumerate(r["history"]):
            if acc and tr[q] - tr[q + 1] != sum(g for _, _, _, g in acc):
                differs += 1
    assert differs >= 1


# ---- float32 against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_float32_decides_like_float64_except_next_to_a_threshold(name):
    """Every term of every mover in every state against the start state: equal, except at pairs whose float64 distance is within
    1e-4 A of a threshold; those are at most 0.1 % of the candidate pairs (section 29's cap)."""
    p64, p32 = H.host_problem(O.batch(name), dtype=np.float64), H.host_problem(O.batch(name), dtype=np.float32)
    n_cand = n_near = bad = 0
    for n in p64.movers:
        for c in range(int(p64.ns[n])):
            cand, near = H.near_threshold(p64, n, c)
            diff = H.pair_terms(p64, n, c) != H.pair_terms(p32, n, c)
            bad += int((diff & ~near).sum())
            n_cand += int(cand.sum())
            n_near += int(near.sum())
    print(f"{name}: {n_cand} candidate pairs, {n_near} within 1e-4 A of a threshold, {bad} other differences")
    assert bad == 0 and n_cand >= 100
    assert n_near <= 1e-3 * n_cand


# ---- the text ----------------------------------------------------------------------------------------------------------------------------
def test_the_csv_text():
    from packppi_amd.analysis import hnet_csv
    ser, asn, ala = rc.resname_to_idx["SER"], rc.resname_to_idx["ASN"], rc.resname_to_idx["ALA"]
    text = hnet_csv(residue_type=[ser, ala, asn, asn], state=[3, -1, 1, 0], e=[[5, -2], [0, 0], [64, -1], [0, 0]],
                    chain=["A", "A", "B", "B"], residue_index=[7, 8, 1, 2])
    assert text == ("chain,residue,name,kind,state,angle,e_before,e_after\n"
                    "A,7,SER,rotor,3,270.0,5,-2\n"
                    "B,1,ASN,flip,1,180.0,64,-1\n"
                    "B,2,ASN,flip,0,0.0,0,0\n")
