"""CPU: the tables of pp_chi_refine and its oracle (tests/refine_oracle.py) against the definition."""
import functools

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc

from . import allatom_oracle as A
from . import polar_oracle as O
from . import refine_oracle as R
from .test_hnet_host import _sep

FIXTURES = ("1BRS", "2FTL", "c24", "c64", "c97")
SEED = 11


def seeded_chi(b, seed=SEED, amp=0.35):
    """The batch's own angles with seeded noise of ``amp`` rad on top."""
    g = torch.Generator().manual_seed(seed)
    chi = b["SC_D"].clone().float()
    return (torch.remainder(chi + amp * torch.randn(chi.shape, generator=g) + np.pi, 2 * np.pi) - np.pi).numpy().astype(np.float32)


# ---- the tables ------------------------------------------------------------------------------------------------------------------------
def test_the_moved_atoms_by_name():
    """The oracle's list, by name on a lysine, and the rule the kernel applies to ``constants.hydrogen_place`` (slots 5 .. 13, and a
    hydrogen whose parent or neighbour entry is one): the same slots on every type, at most the 22 the kernel's LDS holds."""
    tb = A.get_tables()
    lys = rc.resname_to_idx["LYS"]
    names = [tb["names"][lys][s] for s in R.moved_of_type(lys)]
    assert names == ["CG", "CD", "CE", "NZ", "HB2", "HB3", "HG2", "HG3", "HD2", "HD3", "HE2", "HE3", "HZ1", "HZ2", "HZ3"]
    for t in range(20):
        rule = [s for s in range(5, 14) if rc.atom14_names[t][s]]
        rule += [14 + k for k in range(rc.PP_H_MAX) if rc.hydrogen_place[t, k, 0] != 0 and any(5 <= int(v) <= 13 for v in rc.hydrogen_place[t, k, 1:])]
        assert rule == R.moved_of_type(t) and len(rule) <= 22, rc.resnames[t]


def test_ext_bounds_the_farthest_moved_atom_over_a_chi_grid():
    """Every type with a chi, all four angles on a grid of 60 degrees: no moved atom or hydrogen is farther from CA than
    ``refine_extent``."""
    from oracle import ref_cpu as Ref
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(synth.make_complex(24, 5))
    X, bb = b["X"].double()[:, :1], b["BB_D"].double()[:, :1]
    grid = np.deg2rad(np.arange(-180.0, 180.0, 60.0))
    chis = np.stack(np.meshgrid(grid, grid, grid, grid, indexing="ij"), -1).reshape(-1, 4)
    seen = 0
    for t in range(20):
        moved = R.moved_of_type(t)
        if not rc.chi_angles_mask[t].any():
            assert rc.refine_extent[t] == 0
            continue
        n_chi = int(rc.chi_angles_mask[t].sum())
        ch = np.unique(chis[:, :n_chi], axis=0)
        ch = np.concatenate([ch, np.zeros((len(ch), 4 - n_chi))], 1)
        n = len(ch)
        rt = torch.full((1, n), t, dtype=torch.long)
        xyz = Ref.atom14_coords(X.expand(1, n, 14, 3), rt, bb.expand(1, n, 3), torch.from_numpy(ch)[None]).reshape(n, 14, 3).numpy()
        am = np.asarray(rc.atom14_mask[t] != 0, np.float32)[None].repeat(n, 0)
        h, m, _ = A.hydrogens(xyz, am, rt.reshape(-1).numpy(), np.zeros(n, np.int64), list(range(n + 1)))
        heavy, hyd = [s for s in moved if s < 14], [s - 14 for s in moved if s >= 14]
        assert m[:, hyd].all()
        far = max(np.linalg.norm(xyz[:, heavy] - xyz[:, 1:2], axis=-1).max(), np.linalg.norm(h[:, hyd] - xyz[:, 1:2], axis=-1).max())
        print(f"{rc.resnames[t]}: farthest moved atom {far:.3f} A, ext {rc.refine_extent[t]:.3f} A")
        assert 2.0 < far <= rc.refine_extent[t], rc.resnames[t]
        seen += 1
    assert seen == 18


def test_the_angle_of_a_state():
    chi0 = np.array([[3.0, -3.0, 0.5, np.nan]], np.float32)
    d = np.float32(np.deg2rad(16.0))
    assert R.angles(chi0, np.zeros((1, 4), np.int8), d).tobytes() == chi0.tobytes()
    a = R.angles(chi0, np.array([[1, -1, 2, 0]], np.int8), d)
    assert a[0, 0] == np.float32(np.float32(3.0 + np.float32(1 * d)) - R.TWO_PI) and -np.pi <= a[0, 0] < np.pi
    assert a[0, 1] == np.float32(np.float32(-3.0 - d) + R.TWO_PI) and a[0, 2] == np.float32(0.5 + np.float32(2 * d))
    assert np.isnan(a[0, 3])


# ---- the oracle against the definition ---------------------------------------------------------------------------------------------------
# (noise on the batch's own angles in rad, one row in `keep` is free, sweeps allowed): the synthetic complexes are packed at random
# and overlap everywhere, so most of their rows are held and the descent still takes a hundred sweeps
SETUP = {"1BRS": (0.15, 1, 96), "2FTL": (0.15, 1, 96), "c24": (0.2, 1, 160), "c64": (0.2, 3, 160), "c97": (0.2, 3, 160)}


def setup(name):
    b = O.batch(name)
    amp, keep, sweeps = SETUP[name]
    n = b["residue_type"].numel()
    fixed = (np.arange(n) % 7 == 0) if keep == 1 else (np.arange(n) % keep != 1)
    return b, seeded_chi(b, amp=amp), fixed, sweeps


@functools.lru_cache(maxsize=None)
def descent(name, dtype=np.float64, accept="rule"):
    b, chi, fixed, sweeps = setup(name)
    start = R.host_problem(b, chi, dtype=dtype, fixed=fixed)
    p = R.host_problem(b, chi, dtype=dtype, fixed=fixed)
    return start, p, R.optimize(p, sweeps, accept, want_energy=False)


def direct_F(p):
    """F by the definition, scalar by scalar: every pair of counted atoms of a segment of which at least one is a moved atom of a
    mover and which are not moved atoms of the same mover, once.  Pairs farther apart than 4 A (no radius sum, no bond reaches that
    far) are left out before the scalar loop."""
    tot = np.zeros(len(p.seg_off) - 1, np.int64)
    hot = set()
    cut, hba, hbw2, hbg2, band = float(p.cut), float(p.hb_allow), float(p.hbw2), float(p.hbg2), float(p.band)
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
                xi, yi = int(p.cls[n, x]), int(p.cls[j, y])
                if _sep(p, n, x, j, int(y)) <= (4 if (xi | yi) & 4 else 3):
                    continue
                q = p.cur[j, y].astype(np.float64)
                dist2 = float(((q - px) ** 2).sum())
                xh, yh = bool(xi & 1 and yi & 2), bool(xi & 2 and yi & 1)
                t = float(p.cur_w[n, x]) + float(p.cur_w[j, y]) - cut - (hba if xh or yh else 0.0)
                level = sum(1 for k in range(p.bands) if t - k * band > 0 and dist2 <= (t - k * band) ** 2)
                if level:
                    hot.add(n)
                    if p.is_moved[j, y]:
                        hot.add(j)
                if p.is_moved[j, y] and (j, y) < (n, x):
                    continue                                    # counted from the other end
                term = 64 * level
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
    return tot, hot


@pytest.mark.parametrize("name", FIXTURES)
def test_F_equals_a_direct_double_loop(name):
    start, p, r = descent(name)
    f0, hot0 = direct_F(start)
    assert np.array_equal(start.F(), f0) and np.array_equal(f0, r["trace"][:, 0])
    assert np.array_equal(p.F(), direct_F(p)[0]) and np.array_equal(p.F(), r["trace"][:, -1])
    assert int(f0[0]) > 0 and sorted(hot0) == sorted(r["hot"][0])


@pytest.mark.parametrize("name", FIXTURES)
def test_level_one_is_the_serious_overlap_of_the_clashscore(name):
    """The pairs with level >= 1 among the terms of the start state are ``allatom_oracle.clash``'s serious overlaps over the same atoms,
    those with a moved atom of a mover at one end."""
    start, _, _ = descent(name)
    p = start
    ref = A.clash(p.cur[:, :14], p.cur[:, 14:], (p.cur_w[:, 14:] > 0), p.r, p.rtype, p.chain, p.seg_off, p.link_prev, dtype=p.dtype)
    want = {(i, x, j, y) for i, x, j, y in ref["pairs"]
            if (p.is_moved[i, x] or p.is_moved[j, y]) and not (i == j and p.is_moved[i, x] and p.is_moved[j, y])}
    got = set()
    for n in p.movers:
        lo = p.seg_off[int(p.seg_of[n])]
        _, Lv, _, _ = p.pair_terms(n, p.cur, p.cur_w)
        for xk, jr, y in zip(*np.nonzero(Lv >= 1)):
            a, b = (n, p.moved[n][xk]), (lo + int(jr), int(y))
            got.add((*min(a, b), *max(a, b)))
    assert got == want and len(want) >= 3


@pytest.mark.parametrize("name", FIXTURES)
def test_the_descent_is_monotone_in_integers_and_ends_in_a_local_optimum(name):
    start, p, r = descent(name)
    tr, k = r["trace"][0].astype(np.int64), int(r["sweeps"][0])
    assert k >= 1 and r["converged"][0] == 1 and not any(r["history"][k:])
    assert (np.diff(tr[:k + 1]) < 0).all() and (tr[k:] == tr[k]).all()
    for q in range(k):
        acc = r["history"][q]
        assert acc and all(g > 0 for _, _, g in acc)
        assert tr[q] - tr[q + 1] == sum(g for _, _, g in acc), (name, q)
        rows = [n for n, _, _ in acc]
        assert not any(m in r["plist"][n] for n in rows for m in rows), "two accepted movers are partners"
        # nobody without an overlap term proposes
        assert set(r["proposers"][q]) <= set(r["hot"][q])
    for n in p.movers:
        assert all(n in r["plist"][m] for m in r["plist"][n])
    # a local optimum of single steps within max_steps, for every mover that has an overlap left
    assert np.abs(p.steps).max() <= p.max_steps
    sets = p.candidate_sets(p.movers)
    for n in p.movers:
        e0, _, hot = p.energy(n, p.cur, p.cur_w)
        if hot:
            assert all(p.energy(n, sets[c][1], sets[c][2])[0] >= e0 for c in range(1, R.NCAND) if p.exists(n, c)), (name, n)
    # fixed rows and rows that never had an overlap are unmoved, bit for bit
    ever_hot = set().union(*[set(h) for h in r["hot"]])
    for n in range(p.N):
        if p.fixed[n] or n not in ever_hot:
            assert not p.steps[n].any() and r["chi"][n].tobytes() == p.chi0[n].tobytes()
    assert p.fixed.sum() >= 3 and (np.abs(p.steps).sum(1) > 0).sum() >= 1


def test_partners_hold_every_pair_of_movers_whose_moved_atoms_come_within_reach():
    """Over a grid of states of both (every chi at -max_steps, 0, +max_steps): movers whose moved atoms come within reach of each
    other are partners (c24)."""
    start, _, r = descent("c24")
    reach = float(start.reach)
    pos = {}
    for n in start.movers:
        pts = []
        for st in np.stack(np.meshgrid(*[[-3, 0, 3]] * 4, indexing="ij"), -1).reshape(-1, 4):
            ch = start.chi0.copy()
            ch[n] = R.angles(start.chi0[n], st.astype(np.int8), start.delta)
            X, Hh, M = start.build(ch, [n])
            pts.append(np.concatenate([X[n], Hh[n]])[start.moved[n]])
        pos[n] = np.concatenate(pts)
    pairs = 0
    for n in start.movers:
        for m in start.movers:
            if m > n and start.seg_of[m] == start.seg_of[n] and np.linalg.norm(pos[n][:, None] - pos[m][None], axis=-1).min() <= reach:
                assert m in r["plist"][n], (n, m)
                pairs += 1
    assert pairs >= 1, "vacuous: no two movers come within reach"


# ---- float32 against float64 -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FIXTURES)
def test_float32_decides_like_float64_except_next_to_a_band_threshold(name):
    """Every level of every mover at every candidate of the first sweep: equal, except at pairs whose float64 distance is within
    1e-4 A of a band threshold; those are at most 0.1 % of the candidate pairs (allowed pairs of counted atoms within 4 A)."""
    b, chi, _, _ = setup(name)
    p64, p32 = R.host_problem(b, chi, dtype=np.float64), R.host_problem(b, chi, dtype=np.float32)
    s64, s32 = p64.candidate_sets(p64.movers), p32.candidate_sets(p32.movers)
    n_cand = n_near = bad = 0
    for n in p64.movers:
        lo, hi = p64.seg_off[int(p64.seg_of[n])], p64.seg_off[int(p64.seg_of[n]) + 1]
        mv = p64.moved[n]
        for c in range(R.NCAND):
            if not p64.exists(n, c):
                continue
            T64, L64, _, _ = p64.pair_terms(n, s64[c][1], s64[c][2])
            T32, L32, _, _ = p32.pair_terms(n, s32[c][1], s32[c][2])
            pos, pw = s64[c][1][n, mv], s64[c][2][n, mv]
            d = p64.cur[lo:hi][None] - pos[:, None, None]
            dist = np.sqrt((d * d).sum(-1))
            xc, qc = p64.cls[n, mv], p64.cls[lo:hi]
            hbp = (((xc & 1) != 0)[:, None, None] & ((qc & 2) != 0)[None]) | (((xc & 2) != 0)[:, None, None] & ((qc & 1) != 0)[None])
            t = pw[:, None, None] + p64.cur_w[lo:hi][None] - float(p64.cut) - np.where(hbp, float(p64.hb_allow), 0.0)
            ok = p64._allowed_memo[n][mv]
            ok[:, n - lo, mv] = False
            cand = ok & (pw > 0)[:, None, None] & (p64.cur_w[lo:hi] > 0)[None] & (dist <= 4.0)
            near = np.zeros(cand.shape, bool)
            for k in range(p64.bands):
                near |= np.abs(dist - (t - k * float(p64.band))) <= 1e-4
            bad += int(((L64 != L32) & ~near).sum())
            n_cand += int(cand.sum())
            n_near += int((cand & near).sum())
    print(f"{name}: {n_cand} candidate pairs, {n_near} within 1e-4 A of a band threshold, {bad} other differences")
    assert bad == 0 and n_cand >= 1000
    assert n_near <= 1e-3 * n_cand


# ---- the text ----------------------------------------------------------------------------------------------------------------------------
def test_the_csv_text():
    from packppi_amd.analysis import refine_csv
    ser, lys, ala = rc.resname_to_idx["SER"], rc.resname_to_idx["LYS"], rc.resname_to_idx["ALA"]
    steps = np.zeros((2, 3, 4), np.int8)
    steps[0, 0] = [1, 0, 0, 0]
    steps[1, 0] = [-1, 0, 0, 0]
    steps[0, 2] = [0, -2, 0, 1]
    text = refine_csv([ser, ala, lys], steps, (16, 8), [[130, 2], [0, 0], [64, -1]], ["A", "A", "B"], [7, 8, 1])
    assert text == ("chain,residue,name,steps_chi1,steps_chi2,steps_chi3,steps_chi4,rotation_deg,e_before,e_after\n"
                    "A,7,SER,1/-1,0/0,0/0,0/0,24.0,130,2\n"
                    "B,1,LYS,0/0,-2/0,0/0,1/0,48.0,64,-1\n")


# ---- build and ABI -----------------------------------------------------------------------------------------------------------------------
def test_the_binding_takes_what_the_header_declares():
    import ctypes as C
    import os
    import re
    from packppi_amd import build, lib as L
    build.build_library(verbose=False)
    src = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "packppi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    args = [a.strip() for a in re.search(r"pp_status\s+pp_chi_refine\s*\((.*?)\)\s*;", src, flags=re.S).group(1).split(",")]
    want = [C.c_void_p if "*" in a else C.c_float if a.startswith("float ") else C.c_int if a.startswith("int ") else None for a in args]
    assert "pp_chi_refine" in L.SYMBOLS and "pp_refine.hip" in build.SOURCES
    assert L.load().pp_chi_refine.argtypes == want and len(want) == 38


def test_no_kernel_of_the_file_uses_scratch(tmp_path):
    import os
    import re
    import subprocess
    from packppi_amd import build
    out = subprocess.run([build._hipcc(), *build.FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(build.CSRC, "pp_refine.hip"),
                          "-o", str(tmp_path / "pp_refine.o")], capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    lds = dict(zip(names, (int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out))))
    assert len(names) == 7 and len(scratch) == 7 and not any(scratch), list(zip(names, scratch))
    assert max(lds.values()) <= 2 * 9 * 22 * 16 + 2048                 # the candidates' atoms and parents, the separations, the row list
