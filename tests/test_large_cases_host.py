"""CPU: the cases of tests/large_cases.py cannot pass tests/test_large_batches_gpu.py vacuously.

Only the CPU oracles run here.  Each condition below is one a kernel branch needs in order to be exercised beyond its first pass:
overlaps and moves in segments of index 64 and above, movers on both sides of row 1024, a surface point of the first 256 rows that
only a row behind them buries, seed sets whose shell changes when the rows of the third 256-row workgroup go."""
import functools

import numpy as np

from . import allatom_oracle as A
from . import hnet_oracle as H
from . import large_cases as LC
from . import polar_oracle as PO
from . import refine_oracle as R
from . import test_sasa_host as SH
from .test_mutate_host import near_numpy, shell_from_near


def arrays(b):
    X, _, _, chain, offs = PO.arrays(b)
    return X, b["atom_mask"].reshape(-1, 14).numpy(), b["residue_type"].reshape(-1).numpy(), chain, offs


@functools.lru_cache(maxsize=None)
def clash_of_many():
    X, am, rt, chain, offs = arrays(LC.many())
    hx, hm, lp = A.hydrogens(X.astype(np.float64), am, rt, chain, offs)
    return A.clash(X, hx.astype(np.float32), hm, A.default_radius(rt, am), rt, chain, offs, lp)


def test_the_shapes_are_the_ones_the_kernels_branch_on():
    assert LC.N_SEG == 71 > 64 and LC.N_ROWS == 1087 > 1024 and LC.N_ROWS % 8 == 7 and LC.N_ROWS % 16 == 15
    assert LC.N_ROWS % 256 != 0 and LC.N_ROWS % 1024 != 0
    assert LC.LENGTHS[0] == LC.LENGTHS[70] == 1 and LC.LENGTHS[34] == 2 and LC.LENGTHS[35] == 3 and LC.LENGTHS[69] == 24
    assert LC.SEG_1024 == 66 and LC.OFFSETS[66] == 1014 and LC.OFFSETS[67] == 1029
    b = LC.many()
    assert b["seg_offsets_host"] == LC.OFFSETS and b["X"].shape == (1, 1087, 14, 3)
    assert int(b["residue_mask"].sum()) == 1087
    for n in (1024, 1025):
        offs = LC.many_rows(n)["seg_offsets_host"]
        assert offs[-1] == n and offs[:-1] == LC.OFFSETS[:67] and len(offs) - 1 == 67 > 64
    p = LC.many_padded()
    assert p["residue_type"].shape == (68, 17) and 68 * 17 > 1024 and "seg_offsets" not in p
    pad = LC.padding_rows()
    assert pad[:1024].any() and pad[1025:].any() and pad.sum() == 68 * 17 - sum(LC.LENGTHS[i] for i in LC.PADDED_SEGMENTS)
    assert (p["residue_mask"].reshape(-1).numpy() == 0).tolist() == pad.tolist()
    assert LC.long530()["X"].shape == (1, 530, 14, 3) and 530 % 8 == 2 and 530 == 256 + 256 + 18
    for L in (1, 2, 3):
        assert LC.tiny(L)["X"].shape == (1, L, 14, 3)
    xyzr, offs, polar = LC.many_obstacles()
    assert xyzr.shape == (36, 4) and len(offs) == 72 and offs[-1] == 36 and polar.sum() == 18
    assert [s for s in range(71) if offs[s + 1] > offs[s]] == [1, 66, 69]


def test_the_tiny_complexes_hold_movers_of_both_kinds():
    from packppi_amd import constants as rc
    names = {L: [rc.resnames[int(t)] for t in LC.tiny(L)["residue_type"].reshape(-1)] for L in (1, 2, 3)}
    assert names == {1: ["ASN"], 2: ["SER", "CYS"], 3: ["THR", "ASN", "PRO"]}
    kinds = {L: [H.mover_of_type(int(t))[0] for t in LC.tiny(L)["residue_type"].reshape(-1)] for L in (1, 2, 3)}
    assert kinds == {1: [2], 2: [1, 1], 3: [1, 2, 0]}
    for L in (1, 2, 3):
        b = LC.tiny(L)
        assert len(R.host_problem(b, LC.refine_chi(b).numpy()).movers) >= 1
        assert H.optimize(H.host_problem(b, LC.hnet_chi(b).numpy()), 32)["converged"].all()


def test_many_overlaps_in_the_late_segments():
    seg = clash_of_many()["seg"]
    print("segments with an overlap", int((seg[:, 1] >= 1).sum()), "; with a hydrogen in segments 64 ..:", seg[64:, 3].tolist())
    assert (seg[:, 1] >= 1).sum() >= 60
    assert (seg[64:, 3] >= 1).any()
    pol = PO.of_batch(LC.many())["seg"]
    assert (pol[64:, 0] >= 1).any(), "no hydrogen bond in a segment of index 64 or above"


def test_many_the_obstacle_atoms_change_their_three_segments_and_no_other():
    """Clash words, SASA counts and hydrogen-network energies of the oracles with and without the 36 obstacle atoms."""
    b = LC.many()
    xyzr, ooff, polar = LC.many_obstacles()
    X, am, rt, chain, offs = arrays(b)
    hx, hm, lp = A.hydrogens(X.astype(np.float64), am, rt, chain, offs)
    with_ob = A.clash(X, hx.astype(np.float32), hm, A.default_radius(rt, am), rt, chain, offs, lp, obst=xyzr, obst_off=ooff, obst_polar=polar)
    plain = clash_of_many()
    chi = LC.hnet_chi(b).numpy()
    h0 = H.optimize(H.host_problem(b, chi), 32)
    h1 = H.optimize(H.host_problem(b, chi, obst=xyzr, obst_off=ooff, obst_polar=polar), 32)
    s0, s1 = LC.sasa_ref("many", 96), LC.sasa_ref("many", 96, True)
    for s in range(LC.N_SEG):
        lo, hi = offs[s], offs[s + 1]
        differs = (not np.array_equal(with_ob["seg"][s], plain["seg"][s]), not np.array_equal(s0[lo:hi], s1[lo:hi]),
                   not np.array_equal(h0["e"][lo:hi], h1["e"][lo:hi]))
        assert differs == ((s in LC.OBSTACLE_SEGMENTS),) * 3, (s, differs)


def test_many_the_network_sweeps_differ_between_segments_and_late_ones_move():
    b = LC.many()
    ref = H.optimize(H.host_problem(b, LC.hnet_chi(b).numpy()), 32)
    print("sweeps", ref["sweeps"].tolist())
    assert len(set(ref["sweeps"].tolist())) >= 3 and ref["converged"].all()
    assert (ref["sweeps"][64:] >= 1).any()
    assert (ref["trace"][:, 0] != ref["trace"][:, -1]).sum() >= 40


def test_many_refine_has_movers_on_both_sides_of_row_1024_and_moves_behind_it():
    b = LC.many()
    p = R.host_problem(b, LC.refine_chi(b).numpy())
    assert 1023 in p.movers and 1024 in p.movers and len(p.movers) > 512
    ref = R.optimize(p, 1, want_energy=False)
    moved = np.nonzero((ref["steps"] != 0).any(1))[0]
    print(f"movers {len(p.movers)}, with an overlap {len(ref['hot'][0])}, moved {len(moved)}, segments that moved {int((ref['sweeps'] > 0).sum())}")
    assert (moved >= 1024).any() and (ref["sweeps"][64:] >= 1).any()
    b25 = LC.many_rows(1025)
    assert 1024 in R.host_problem(b25, LC.refine_chi(b25).numpy()).movers
    b24 = LC.many_rows(1024)
    assert 1023 in R.host_problem(b24, LC.refine_chi(b24).numpy()).movers


def test_long530_a_point_of_the_first_walk_pass_is_buried_from_the_second_only():
    """SASA at P = 16, probe 1.4, float32 restatement: with the atoms of rows 256 .. 529 gone (radius 0: no points, bury nobody)
    some count of a row in 0 .. 255 changes."""
    from packppi_amd.analysis import sphere_points
    X, radius, chain = SH.arrays(LC.long530())
    full = LC.sasa_ref("long530", 16)
    cut = radius.copy()
    cut[256:] = 0
    front = SH.restate(X, cut, chain, [0, 530], sphere_points(16), 1.4)
    rows = int((full[:256] != front[:256]).any((1, 2)).sum())
    print(f"rows below 256 with a point only a row at or above 256 buries: {rows}")
    assert rows >= 1 and (front[:256] >= full[:256]).all()


def test_long530_the_seed_sets_reach_across_the_third_workgroup():
    b = LC.long530()
    X, am, rt, chain, offs = arrays(b)
    for mode in ("ca", "atom"):
        near = near_numpy(X, [0, 530], 10.0, mode, am)[0]      # the pair matrix of the first 512 rows alone is its corner
        for name, seeds in LC.long530_seed_sets().items():
            for other in (None, chain):
                whole, _ = shell_from_near([near], seeds, [0, 530], other)
                front, _ = shell_from_near([near[:512, :512]], seeds[:512], [0, 512], None if other is None else other[:512])
                changed = int((whole[:512] != front).sum()) + int(whole[512:].sum())
                assert changed >= 1, (name, mode, other is not None)
