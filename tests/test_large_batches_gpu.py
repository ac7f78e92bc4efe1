"""The structure stages beyond 1024 rows, 64 segments and 256-row walks, and at one, two and three residues.

Shell masks, SASA, disulfides, polar contacts, hydrogens and clashscore, hydrogen-bond networks and chi refinement on the cases of
tests/large_cases.py, each against the oracle and with the comparison helpers of its own suite (test_allatom_gpu, test_polar_gpu,
test_sasa_gpu, test_shell_gpu, test_disulfide_gpu, test_hnet_gpu, test_refine_gpu).  No bound is new: integer outputs are compared
as bytes, ``hxyz`` and the candidates within ``hxyz_tolerance``, areas within ``AREA_RTOL``, disulfide reports within
``oracle_tolerance``.  tests/test_large_cases_host.py shows on the CPU that the cases reach the branches they are here for.  Nothing
measured on the device enters a bound."""
import functools

import numpy as np
import pytest
import torch

from . import disulfide_oracle as DO
from . import large_cases as LC
from . import polar_oracle as PO
from . import test_allatom_gpu as AA
from . import test_disulfide_gpu as DG
from . import test_hnet_gpu as HN
from . import test_polar_gpu as PG
from . import test_refine_gpu as RF
from . import test_sasa_gpu as SG
from . import test_sasa_host as SH
from . import test_shell_gpu as SHG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def host(t, *shape):
    return t.reshape(*shape).cpu().numpy()


@functools.lru_cache(maxsize=None)
def shared_ctx(name):
    """One context per case for the calls that leave it as they found it (no obstacle atoms are ever installed here)."""
    return AA.new_ctx(LC.CASES[name]())


# ---- one call of a stage against its oracle --------------------------------------------------------------------------------------------
def check_clash(b, ctx, what, **ref_kw):
    res = ctx.clashscore(**({"obst_polar": torch.from_numpy(ref_kw["obst_polar"])} if "obst_polar" in ref_kw else {}))
    hx, hm, lp = AA.check_hydrogens(res, b, what=what)
    ref = AA.reference(b, res, **ref_kw)
    got = AA.words(res)
    print(f"{what}: {got['res'].shape[0]} rows, {got['seg'].shape[0]} segments, words that differ {[int((got[k] != ref[k]).sum()) for k in AA.KEYS]}")
    AA.assert_same_bytes(got, ref, what)
    assert got["seg"].shape == (len(LC.offsets(b)) - 1, 8)
    assert np.allclose(res.clashscore.cpu().numpy(), AA.A.clashscore(ref["seg"]), rtol=0, atol=1e-9)
    h = ctx.hydrogens()
    assert torch.equal(h.hxyz, res.hxyz) and torch.equal(h.hmask, res.hmask) and torch.equal(h.link_prev, res.link_prev)
    assert ctx.saturated() == 0
    return res, got, ref, hm


def check_polar(b, ctx, ref, what):
    got = PG.words(ctx.polar())
    print(f"{what}: {ref['res'].shape[0]} rows, {ref['seg'].shape[0]} segments, words that differ {[int((got[k] != ref[k]).sum()) for k in PG.KEYS]}")
    PG.assert_same_bytes(got, ref, what)
    return got


def check_sasa(b, ctx, c32, P, what):
    got, res = SG.device_counts(ctx, n_points=P)
    X, radius, chain = SH.arrays(b)
    offs = LC.offsets(b)
    assert got.dtype == np.int32 and got.shape == c32.shape, what
    print(f"{what}: {got.shape[0]} rows, {len(offs) - 1} segments, P = {P}, words that differ {int((got != c32).sum())}")
    assert got.tobytes() == c32.tobytes(), (what, int((got != c32).sum()))
    want = SH.area_fp64(got, radius, 1.4, P)
    area = host(res.area, -1, 4).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.nanmax(np.where(want > 0, np.abs(area - want) / want, 0.0))) if want.size else 0.0
    print(f"{what}: largest relative area error {worst:.3g} (bound {SG.AREA_RTOL:.3g})")
    assert (np.abs(area - want) <= SG.AREA_RTOL * np.abs(want)).all(), what
    seg = res.seg_area.cpu().numpy()
    assert seg.dtype == np.float64 and seg.shape == (len(offs) - 1, 4)
    for s, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        assert np.allclose(seg[s], area[lo:hi].sum(0), rtol=1e-12, atol=0), (what, s)
    return got, res


def check_disulfides(b, ctx, what, chi=None):
    chi = b["SC_D"] if chi is None else chi
    hb, offs = DG.host(b), LC.offsets(b)
    r32 = DO.solve(hb, offs, chi=chi.numpy(), dtype=np.float32)
    r64 = DO.solve(hb, offs, chi=chi.numpy(), dtype=np.float64)
    tol, diff = DG.oracle_tolerance(r32, r64)
    res = ctx.disulfides(chi=chi)
    partner, report, _ = DG.check_against(res, r32, tol, chi.numpy())
    rows = [a for a, _ in r32["bonded"]]
    dev = float(np.abs(report[rows] - r32["report"][rows]).max()) if rows else 0.0
    print(f"{what}: {len(DO.eligible(hb).nonzero()[0])} cysteines, {len(r32['emin'])} candidate pairs, {len(rows)} bridges; report within "
          f"{dev:.3g} of the float32 oracle (bound {tol:.3g})")
    assert res.count.shape == (len(offs) - 1,)
    return res, r32


# ---- what the cases found: a context without a network has no K -------------------------------------------------------------------------------
def test_a_geometry_context_packs_a_short_complex_with_a_long_one():
    """pp_complex_prepare_packed refused complexes shorter than 32 rows next to longer ones under every plan, although only the
    network has the K = min(32, L) the rule is about (a plan WITH weights still refuses:
    test_hip_parity.py::test_packed_batch_equals_per_complex).  16 and 64 rows: each gets the words of its own run."""
    from packppi_amd.batch import pack
    parts = [LC.segment(1), PO.batch("c64")]
    b = pack(parts)
    assert b["seg_offsets_host"] == [0, 16, 80]
    ctx = AA.new_ctx(b)
    got = PG.words(ctx.polar())
    PG.assert_same_bytes(got, PO.of_batch(b), "16 + 64 rows")
    cl = AA.words(ctx.clashscore())
    for s, (lo, hi) in enumerate(((0, 16), (16, 80))):
        alone = AA.new_ctx(parts[s])
        pa, ca = PG.words(alone.polar()), AA.words(alone.clashscore())
        for k in PG.KEYS[:3]:
            assert got[k][lo:hi].tobytes() == pa[k].tobytes(), (s, k)
        for k in AA.KEYS[:3]:
            assert cl[k][lo:hi].tobytes() == ca[k].tobytes(), (s, k)
        assert got["seg"][s].tobytes() == pa["seg"][0].tobytes() and cl["seg"][s].tobytes() == ca["seg"][0].tobytes()


# ---- many(): 71 segments, 1087 rows -----------------------------------------------------------------------------------------------------------
def test_many_clashscore_and_hydrogens():
    res, got, ref, _ = check_clash(LC.many(), shared_ctx("many"), "many")
    assert (ref["seg"][:, 1] >= 1).sum() >= 60 and (ref["seg"][64:, 3] >= 1).any()


def test_many_polar():
    got = check_polar(LC.many(), shared_ctx("many"), LC.polar_ref("many"), "many")
    assert (got["seg"][64:, 0] >= 1).any()


def test_many_sasa():
    check_sasa(LC.many(), shared_ctx("many"), LC.sasa_ref("many", 96), 96, "many")


def test_many_shell():
    """Both modes, with and without PP_SHELL_OTHER_CHAIN, three radii, the batch's X and rebuilt atoms: every row a seed (a workgroup
    of 256 rows spans up to 17 segments and walks more than 256 seed rows), one seed in the segment of row 1024, none."""
    b = LC.many().to(DEV)
    assert SHG._run_matrix(b, LC.OFFSETS, LC.many_seed_sets()) == 2 * 2 * 3 * 3 * 2


def test_many_disulfides():
    check_disulfides(LC.many(), shared_ctx("many"), "many")


def test_many_hydrogen_network():
    b = LC.many()
    ctx, res, ref = HN.run_and_check(b, LC.hnet_chi(b), "many", ctx=shared_ctx("many"))
    assert len(set(ref["sweeps"].tolist())) >= 3 and (ref["sweeps"][64:] >= 1).any() and ref["converged"].all()
    assert res.trace.shape == (71, 33) and res.n_movers.shape == (71,)


@pytest.mark.parametrize("max_sweeps", [1, 3])
def test_many_refine(max_sweeps):
    b = LC.many()
    ctx, res, ref, p = RF.run_and_check(b, LC.refine_chi(b), f"many, {max_sweeps} sweep(s)", ctx=shared_ctx("many"), max_sweeps=max_sweeps,
                                        cands=max_sweeps == 1)
    assert 1023 in p.movers and 1024 in p.movers
    moved = np.nonzero((ref["steps"] != 0).any(1))[0]
    assert (moved >= 1024).any() and (ref["sweeps"][64:] >= 1).any()
    assert res.trace.shape == (1, 71, max_sweeps + 1)


# ---- alone, packed, twice ---------------------------------------------------------------------------------------------------------------------
def _rel(partner, offs):
    """Disulfide partners as rows of their own segment."""
    seg = np.searchsorted(np.asarray(offs), np.arange(len(partner)), side="right") - 1
    return np.where(partner >= 0, partner - np.asarray(offs)[seg], -1)


def out_clash(ctx, b, chi_h, chi_r):
    r = ctx.clashscore()
    w = AA.words(r)
    return dict(partners=w["partners"], n_clash=w["n_clash"], res=w["res"], hxyz=host(r.hxyz, -1, 39), hmask=host(r.hmask, -1, 13)), dict(seg=w["seg"])


def out_polar(ctx, b, chi_h, chi_r):
    w = PG.words(ctx.polar())
    return {k: w[k] for k in PG.KEYS[:3]}, dict(seg=w["seg"])


def out_sasa(ctx, b, chi_h, chi_r):
    got, res = SG.device_counts(ctx)
    return dict(counts=got, area=host(res.area, -1, 4)), dict(seg_area=res.seg_area.cpu().numpy())


def out_shell(ctx, b, chi_h, chi_r):
    rows, segs = {}, {}
    n = b["residue_type"].numel()
    for mode in ("ca", "atom"):
        for other in (False, True):
            sh, cnt = ctx.shell(torch.ones(1, n, dtype=torch.uint8), radius=8.0, mode=mode, other_chain=other, want_count=True)
            rows[(mode, other)], segs[(mode, other)] = host(sh, -1).astype(np.uint8), cnt.cpu().numpy()
    return rows, segs


def out_disulfides(ctx, b, chi_h, chi_r):
    r = ctx.disulfides(chi=b["SC_D"])
    return dict(partner=_rel(r.partner.cpu().numpy(), LC.offsets(b)), report=r.report.cpu().numpy(), chi=host(r.chi, -1, 4)), dict(count=r.count.cpu().numpy())


def out_hnet(ctx, b, chi_h, chi_r):
    r = ctx.hbond_optimize(chi=chi_h.to(DEV), want_candidates=True)
    w = HN.words(r)
    rows = {k: w[k] for k in ("state", "e", "hb", "energy")}
    rows.update(hxyz=host(r.hxyz, -1, 39), xyz=host(r.xyz, -1, 42), chi=host(r.chi, -1, 4))
    return rows, dict(trace=w["trace"], sweeps=w["sweeps"], converged=w["converged"], n_movers=r.n_movers.cpu().numpy())


def out_refine(ctx, b, chi_h, chi_r):
    r = ctx.refine_allatom(chi_r.to(DEV), deltas_deg=(16,), max_sweeps=3, want_candidates=True)
    w = RF.words(r)
    rows = {k: w[k] for k in ("steps", "e", "energy", "cand_mask")}
    rows.update(chi=host(r.chi, -1, 4), hxyz=host(r.hxyz, -1, 39))
    return rows, dict(trace=w["trace"], sweeps=w["sweeps"], converged=w["converged"])


STAGES = dict(clashscore=out_clash, polar=out_polar, sasa=out_sasa, shell=out_shell, disulfides=out_disulfides, hbond_optimize=out_hnet,
              refine_allatom=out_refine)


@functools.lru_cache(maxsize=None)
def plain_many(stage):
    b = LC.many()
    return STAGES[stage](shared_ctx("many"), b, LC.hnet_chi(b), LC.refine_chi(b))


@pytest.mark.parametrize("stage", sorted(STAGES))
def test_a_segment_gets_the_bytes_of_its_own_run_and_a_second_call_the_same(stage):
    """Segments 0 and 70 (one row, first and last), 34 (two rows), 1, 66 (it holds row 1024) and 69 (24 rows) of ``many()``."""
    b = LC.many()
    chi_h, chi_r = LC.hnet_chi(b), LC.refine_chi(b)
    rows, segs = plain_many(stage)
    again_rows, again_segs = STAGES[stage](shared_ctx("many"), b, chi_h, chi_r)
    for k in rows:
        assert rows[k].shape[0] == LC.N_ROWS and rows[k].tobytes() == again_rows[k].tobytes(), (stage, k, "two runs")
    for k in segs:
        assert segs[k].shape[0] == LC.N_SEG and segs[k].tobytes() == again_segs[k].tobytes(), (stage, k, "two runs")
    for s in LC.ALONE_SEGMENTS:
        sb = LC.segment(s)
        lo, hi = LC.OFFSETS[s], LC.OFFSETS[s + 1]
        a_rows, a_segs = STAGES[stage](AA.new_ctx(sb), sb, LC.rows_of(chi_h, b, s), LC.rows_of(chi_r, b, s))
        for k in rows:
            assert rows[k][lo:hi].tobytes() == a_rows[k].tobytes(), (stage, s, k)
        for k in segs:
            assert segs[k][s].tobytes() == a_segs[k][0].tobytes(), (stage, s, k)


# ---- the compaction pass exactly full, and a second pass of one row -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1024, 1025])
def test_many_rows_at_the_compaction_boundary(n):
    b = LC.many_rows(n)
    ctx = AA.new_ctx(b)
    HN.run_and_check(b, LC.hnet_chi(b), f"{n} rows", ctx=ctx)
    _, res, ref, p = RF.run_and_check(b, LC.refine_chi(b), f"{n} rows", ctx=ctx, max_sweeps=1)
    assert (n - 1) in p.movers and res.trace.shape == (1, 67, 2)


# ---- padded [68][17]: the uniform table, padding rows on both sides of row 1024 ---------------------------------------------------------------------
def test_many_padded():
    b = LC.many_padded()
    pad = LC.padding_rows()
    ctx = AA.new_ctx(b)
    res, got, ref, hm = check_clash(b, ctx, "padded [68][17]")
    assert (got["res"][pad] == 0).all() and (got["partners"][pad] == -1).all() and (got["n_clash"][pad] == 0).all() and (hm[pad] == 0).all()
    assert (host(res.hxyz, -1, 39)[pad] == 0).all()
    _, hres, href = HN.run_and_check(b, LC.hnet_chi(b), "padded [68][17]", ctx=ctx)
    st = host(hres.state, -1)
    assert (st[pad] == -1).all() and (host(hres.e, -1, 2)[pad] == 0).all() and (host(hres.hmask, -1, 13)[pad] == 0).all()
    assert (st >= 0).sum() >= 200 and len(set(href["sweeps"].tolist())) >= 3


# ---- obstacle atoms for three of the 71 segments ------------------------------------------------------------------------------------------------
def test_many_with_obstacles_for_three_segments():
    b = LC.many()
    xyzr, ooff, polar = LC.many_obstacles()
    ctx = AA.new_ctx(b)
    ctx.set_obstacles(torch.from_numpy(xyzr), LC.obstacle_ranges(), polar=polar)
    res, got, ref, _ = check_clash(b, ctx, "many with obstacles", obst=xyzr, obst_off=ooff, obst_polar=polar)
    counts, _ = check_sasa(b, ctx, LC.sasa_ref("many", 96, True), 96, "many with obstacles")
    chi = LC.hnet_chi(b)
    _, hres, href = HN.run_and_check(b, chi, "many with obstacles", ctx=ctx, ref_kw=dict(obst=xyzr, obst_off=ooff, obst_polar=polar))
    hw = HN.words(hres)
    plain = {"clash": plain_many("clashscore"), "sasa": plain_many("sasa"), "hnet": plain_many("hbond_optimize")}
    for s in range(LC.N_SEG):
        lo, hi = LC.OFFSETS[s], LC.OFFSETS[s + 1]
        same = (got["seg"][s].tobytes() == plain["clash"][1]["seg"][s].tobytes() and got["n_clash"][lo:hi].tobytes() == plain["clash"][0]["n_clash"][lo:hi].tobytes(),
                counts[lo:hi].tobytes() == plain["sasa"][0]["counts"][lo:hi].tobytes(),
                all(hw[k][lo:hi].tobytes() == plain["hnet"][0][k][lo:hi].tobytes() for k in ("state", "e", "hb", "energy"))
                and hw["trace"][s].tobytes() == plain["hnet"][1]["trace"][s].tobytes())
        assert same == ((s not in LC.OBSTACLE_SEGMENTS),) * 3, (s, same)


# ---- long530: one segment, three 256-row passes -----------------------------------------------------------------------------------------------------
def test_long530_sasa():
    check_sasa(LC.long530(), shared_ctx("long530"), LC.sasa_ref("long530", 16), 16, "long530")


def test_long530_polar():
    check_polar(LC.long530(), shared_ctx("long530"), LC.polar_ref("long530"), "long530")


def test_long530_clashscore():
    check_clash(LC.long530(), shared_ctx("long530"), "long530")


def test_long530_shell():
    """One seed at row 520, seeds on rows 256 .. 511 only, every row: the segment spans three workgroups and its seed walk three passes."""
    b = LC.long530().to(DEV)
    assert SHG._run_matrix(b, [0, 530], LC.long530_seed_sets()) == 2 * 2 * 3 * 3 * 2


def test_long530_hydrogen_network():
    b = LC.long530()
    ctx, res, ref = HN.run_and_check(b, LC.hnet_chi(b), "long530", ctx=shared_ctx("long530"))
    assert ref["sweeps"][0] >= 2 and (ref["state"] >= 0).sum() >= 100


def test_long530_refine():
    """The restatement's time is the candidate energies of the 406 movers before the first sweep: fewer sweeps would not shorten it."""
    b = LC.long530()
    ctx, res, ref, p = RF.run_and_check(b, LC.refine_chi(b), "long530", ctx=shared_ctx("long530"), max_sweeps=1, cands=False)
    assert len(p.movers) >= 300 and (ref["steps"] != 0).any()


# ---- one, two and three residues ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3])
def test_tiny_every_stage(L):
    b = LC.tiny(L)
    name = f"tiny{L}"
    ctx = AA.new_ctx(b)
    check_clash(b, ctx, name)
    check_polar(b, ctx, PO.of_batch(b), name)
    check_sasa(b, ctx, LC.sasa_ref(name, 96), 96, name)
    SHG._run_matrix(b.to(DEV), [0, L], SHG._seed_sets(0, L, L))
    check_disulfides(b, ctx, name)
    _, hres, href = HN.run_and_check(b, LC.hnet_chi(b), name, ctx=ctx)
    assert (href["state"] >= 0).sum() >= 1, "no mover"
    _, rres, rref, p = RF.run_and_check(b, LC.refine_chi(b), name, ctx=ctx, max_sweeps=3)
    assert len(p.movers) >= 1


def test_one_cysteine_alone_has_no_bridge():
    """N = 1: the candidate list of pp_disulfide_close has its floor of one entry and nothing to put in it."""
    from packppi_amd import constants as rc
    b = LC.tiny(1).clone()
    b["residue_type"] = torch.full_like(b["residue_type"], DO.CYS)
    b["atom_mask"] = torch.as_tensor(np.asarray(rc.atom14_mask, np.float32)[DO.CYS]).reshape(b["atom_mask"].shape)
    assert DO.eligible(DG.host(b)).tolist() == [True]
    res, r32 = check_disulfides(b, AA.new_ctx(b), "one cysteine")
    assert res.count.tolist() == [0] and res.partner.tolist() == [-1] and not bool(res.report.any()) and res.bonds() == []


# ---- bridges behind row 1024 ----------------------------------------------------------------------------------------------------------------------
def test_disulfides_behind_row_1024():
    from packppi_amd.batch import pack
    b = pack([LC.segment(i) for i in range(LC.N_SEG)] + [DG.batch("2FTL", "I"), DG.batch("2FTL")])
    offs = b["seg_offsets_host"]
    assert offs[71] == 1087 and offs[72] == 1087 + 58 and offs[73] == 1087 + 58 + 280
    res, r32 = check_disulfides(b, AA.new_ctx(b), "many + 2FTL chain I + 2FTL")
    assert r32["count"][71] == 3 and r32["count"][72] == 9
    count = res.count.cpu().numpy()
    assert count[71] == 3 and count[72] == 9 and count.tolist() == r32["count"].tolist()
    partner = res.partner.cpu().numpy()
    seg = np.searchsorted(np.asarray(offs), np.arange(len(partner)), side="right") - 1
    bonded = np.nonzero(partner >= 0)[0]
    assert len(bonded) == 2 * int(count.sum()) and (seg[partner[bonded]] == seg[bonded]).all(), "a bridge across two segments"
    assert (bonded >= 1087).sum() == 24
