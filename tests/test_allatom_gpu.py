"""Explicit hydrogens and the all-atom clashscore on the device, through the C ABI (pp_hydrogens, pp_clashscore).

Reference: tests/allatom_oracle.py (brute force over all atoms of a segment, its own literal chemistry).  ``hmask`` and ``link_prev``
must have its BYTES.  ``hxyz`` must lie within 1e-5 A + 2 ulp32(largest |coordinate|) of the float64 oracle: the direction is built
from differences to the parent, so the only error of the size of the coordinates is the final add.  The four integer arrays of
pp_clashscore must have the BYTES of the float32 restatement fed the device's own ``hxyz``.  The oracle has no row filter, so every
comparison is also the filter against the unfiltered count (c97 has more rows than one 64-row filter step).  Nothing measured on
the device enters a bound."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from . import allatom_oracle as A
from . import polar_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
KEYS = ("partners", "n_clash", "res", "seg")


def new_ctx(batch):
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    gb = batch.to(DEV)
    ctx = Context(geometry_plan(torch.device(DEV)), gb)
    ctx._keep = gb
    return ctx


def words(res):
    return dict(partners=res.partners.reshape(-1, 27, 4).cpu().numpy(), n_clash=res.n_clash.reshape(-1, 27, 2).cpu().numpy(),
                res=res.res.reshape(-1, 4).cpu().numpy(), seg=res.seg.cpu().numpy())


def assert_same_bytes(got, want, what=""):
    for k in KEYS:
        assert got[k].dtype == np.int32 and got[k].shape == want[k].shape, (what, k)
        assert got[k].tobytes() == want[k].tobytes(), (what, k, int((got[k] != want[k]).sum()))


def arrays(b):
    """(X f32 [N, 14, 3], atom_mask [N, 14], residue_type [N], chain [N], segment table) of a batch."""
    X, _, _, chain, offs = O.arrays(b)
    return X, b["atom_mask"].reshape(-1, 14).numpy(), b["residue_type"].reshape(-1).numpy(), chain, offs


def hxyz_tolerance(X):
    big = np.float32(np.abs(X[np.isfinite(X)]).max())
    return 1e-5 + 2 * float(np.spacing(big))


def check_hydrogens(h, b, xyz=None, link=None, what=""):
    """The device's hydrogens against the float64 oracle; returns (hxyz, hmask, link_prev) of the device on the host."""
    X, am, rt, chain, offs = arrays(b)
    if xyz is not None:
        X = np.asarray(xyz, np.float32).reshape(-1, 14, 3)
    want_xyz, want_mask, want_lp = A.hydrogens(X.astype(np.float64), am, rt, chain, offs, link=link)
    hx, hm, lp = h.hxyz.reshape(-1, 13, 3).cpu().numpy(), h.hmask.reshape(-1, 13).cpu().numpy(), h.link_prev.reshape(-1).cpu().numpy()
    assert hm.dtype == np.uint8 and hm.tobytes() == want_mask.tobytes(), (what, int((hm != want_mask).sum()))
    assert lp.dtype == np.uint8 and lp.tobytes() == want_lp.tobytes(), what
    err = float(np.abs(hx - want_xyz).max())
    print(f"{what}: {int(hm.sum())} hydrogens, {int(lp.sum())} peptide links, largest error {err:.3g} A (bound {hxyz_tolerance(X):.3g})")
    assert np.isfinite(hx).all() and err <= hxyz_tolerance(X), (what, err)
    assert (hx[hm == 0] == 0).all()
    return hx, hm, lp


def reference(b, res, xyz=None, link=None, rotatable="skip", **kw):
    """The float32 restatement of pp_clashscore fed the DEVICE's hydrogens."""
    X, am, rt, chain, offs = arrays(b)
    if xyz is not None:
        X = np.asarray(xyz, np.float32).reshape(-1, 14, 3)
    return A.clash(X, res.hxyz.reshape(-1, 13, 3).cpu().numpy(), res.hmask.reshape(-1, 13).cpu().numpy(),
                   A.default_radius(rt, am, rotatable), rt, chain, offs, res.link_prev.reshape(-1).cpu().numpy(), link=link, **kw)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def _padded():
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_data
    return collate([protein_to_data(O.protein("c40")), protein_to_data(O.protein("c36"))])


def _pack3():
    from packppi_amd.batch import pack
    return pack([O.batch("c97"), O.batch("c65"), O.batch("c97")])


SINGLES = ("c24", "c64", "c97", "three_chains", "1BRS", "2FTL", "damaged64")
CASES = {**{n: functools.partial(O.batch, n) for n in SINGLES}, "padded": _padded, "pack3": _pack3}


@pytest.mark.parametrize("name", sorted(CASES))
def test_hydrogens_and_words_against_the_oracle(name):
    b = CASES[name]()
    ctx = new_ctx(b)
    res = ctx.clashscore()
    hx, hm, lp = check_hydrogens(res, b, what=name)
    ref = reference(b, res)
    got = words(res)
    print(f"{name}: seg {ref['seg'].tolist()}, words that differ {[int((got[k] != ref[k]).sum()) for k in KEYS]}")
    assert ref["seg"][:, 1].min() >= 1 and ref["seg"][:, 3].min() >= 1, "vacuous: no overlap, or none with a hydrogen"
    assert_same_bytes(got, ref, name)
    assert np.allclose(res.clashscore.cpu().numpy(), A.clashscore(ref["seg"]), rtol=0, atol=1e-9)
    assert ctx.saturated() == 0
    X, am, rt, chain, offs = arrays(b)
    pro = rt == 14
    assert (hm[rt == 20] == 0).all()
    if name in ("1BRS", "2FTL", "c97"):
        assert (pro & (lp != 0)).sum() >= 1                   # a proline behind another residue: linked, and its N has no hydrogen
        names = [A.get_tables()["names"][14][14 + k] for k in range(13)]
        assert "H" not in names and names[0] == "HA"
    if name == "damaged64":
        assert (am == 0).sum() >= 20 and hm.sum() < A.hydrogens(X.astype(np.float64), np.ones_like(am), rt, chain, offs)[1].sum()
    if name == "padded":
        assert (got["res"][36 + 40:] == 0).all() and (got["partners"][36 + 40:] == -1).all() and (hm[36 + 40:] == 0).all()
    # the hydrogens alone are the same words
    h = ctx.hydrogens()
    assert torch.equal(h.hxyz, res.hxyz) and torch.equal(h.hmask, res.hmask) and torch.equal(h.link_prev, res.link_prev)


def test_keeping_the_rotatable_hydrogens_and_dropping_the_lists():
    b = O.batch("1BRS")
    ctx = new_ctx(b)
    keep = ctx.clashscore(rotatable="keep")
    ref = reference(b, keep, rotatable="keep")
    assert_same_bytes(words(keep), ref, "keep")
    skip = ctx.clashscore(want_partners=False)
    assert skip.partners is None and int(keep.seg[0, 0]) > int(skip.seg[0, 0])
    sref = reference(b, skip)
    for k in KEYS[1:]:
        assert skip[k].reshape(sref[k].shape).cpu().numpy().tobytes() == sref[k].tobytes()
    wide = ctx.clashscore(cut=0.2, hb_allow=0.0)
    assert_same_bytes(words(wide), reference(b, wide, cut=0.2, hb_allow=0.0), "cut 0.2, no allowance")
    assert int(wide.seg[0, 1]) > int(skip.seg[0, 1])
    with pytest.raises(ValueError, match="rotatable"):
        ctx.clashscore(rotatable="optimise")


def test_decoys_at_three_chi_sets_and_chi_against_xyz():
    from packppi_amd.batch import replicate
    b = replicate(O.batch("c24"), 3)
    ctx = new_ctx(b)
    g = torch.Generator().manual_seed(5)
    chi = ((torch.rand(1, 72, 4, generator=g) * 2 - 1) * np.pi).to(DEV)
    xyz = ctx.atom14(chi)
    ra, rc_ = ctx.clashscore(chi=chi), ctx.clashscore(xyz=xyz)
    assert_same_bytes(words(ra), words(rc_), "chi= against xyz=")
    assert torch.equal(ra.hxyz, rc_.hxyz)
    host = xyz.reshape(-1, 14, 3).cpu().numpy()
    check_hydrogens(ra, b, xyz=host, what="decoys")
    ref = reference(b, ra, xyz=host)
    assert_same_bytes(words(ra), ref, "decoys")
    assert len({ref["n_clash"][24 * d:24 * d + 24].tobytes() for d in range(3)}) == 3
    assert not np.array_equal(words(ra)["res"], words(ctx.clashscore())["res"])


def test_a_segment_gets_the_same_words_alone_packed_and_as_a_decoy():
    from packppi_amd.batch import replicate
    alone = {}
    for n in ("c97", "c65"):
        r = new_ctx(O.batch(n)).clashscore()
        alone[n] = (words(r), r.hxyz.reshape(-1, 39).cpu().numpy(), r.hmask.reshape(-1, 13).cpu().numpy())
    ctx = new_ctx(_pack3())
    r1, r2 = ctx.clashscore(), ctx.clashscore()
    packed = words(r1)
    assert_same_bytes(packed, words(r2), "two runs")
    assert torch.equal(r1.hxyz, r2.hxyz)
    hx = r1.hxyz.reshape(-1, 39).cpu().numpy()
    for (lo, hi), n, s in (((0, 97), "c97", 0), ((97, 162), "c65", 1), ((162, 259), "c97", 2)):
        for k in KEYS[:3]:
            assert packed[k][lo:hi].tobytes() == alone[n][0][k].tobytes(), (n, s, k)
        assert packed["seg"][s].tobytes() == alone[n][0]["seg"][0].tobytes()
        assert hx[lo:hi].tobytes() == alone[n][1].tobytes()
    dr = new_ctx(replicate(O.batch("c65"), 3)).clashscore()
    dec = words(dr)
    for d in range(3):
        for k in KEYS[:3]:
            assert dec[k][65 * d:65 * d + 65].tobytes() == alone["c65"][0][k].tobytes()
        assert dec["seg"][d].tobytes() == alone["c65"][0]["seg"][0].tobytes()


@pytest.mark.parametrize("rot_seed,shift", [(None, (1e4, -1e4, 1e4)), (1, (3.0, -7.0, 11.0)), (2, (1e4, 1e4, -1e4))])
def test_far_from_the_origin_and_under_a_rotation(rot_seed, shift):
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(synth.rigid_motion(O.protein("c64"), rot_seed, np.array(shift)))
    res = new_ctx(b).clashscore()
    check_hydrogens(res, b, what=f"rotation {rot_seed}, shift {shift}")
    assert_same_bytes(words(res), reference(b, res), "moved")


# ---- hand-made rows ------------------------------------------------------------------------------------------------------------------------
def test_a_chain_break_inside_a_chain_has_no_hydrogen_on_n_and_no_exclusion():
    from packppi_amd.batch import Batch
    b = O.batch("c64")
    X = b["X"].clone()
    k = 20                                                   # inside the first chain (rows 0 .. 31)
    assert int(b["chain_indices"].reshape(-1)[k]) == int(b["chain_indices"].reshape(-1)[k - 1])
    bond = X[0, k, 0] - X[0, k - 1, 2]
    X[0, k:32] += bond / bond.norm()                         # C - N grows from 1.33 to 2.33 A: no peptide bond, and a serious overlap
    nb = Batch({**dict(b.items()), "X": X})
    res = new_ctx(nb).clashscore()
    hx, hm, lp = check_hydrogens(res, nb, what="chain break")
    assert lp[k] == 0 and hm[k, 0] == 0 and lp[k - 1] == 1 and lp[k + 1] == 1
    ref = reference(nb, res)
    assert_same_bytes(words(res), ref, "chain break")
    assert (k - 1, 2, k, 0) in ref["pairs"], "vacuous: C and N across the break do not overlap"
    whole = reference(b, new_ctx(b).clashscore())
    assert (k - 1, 2, k, 0) not in whole["pairs"]            # the same two atoms, bonded: excluded


def test_atoms_exactly_in_line_drop_the_hydrogen():
    from packppi_amd.batch import Batch
    b = O.batch("c24")
    X = b["X"].clone()
    rt = b["residue_type"].reshape(-1)
    k = next(r for r in range(2, 11) if int(rt[r]) != 14)   # not a proline: its N has a hydrogen to lose
    n = torch.round(X[0, k, 0] * 4) / 4                      # exact arithmetic: the two unit vectors cancel to 0
    X[0, k, 0], X[0, k, 1], X[0, k - 1, 2] = n, n + torch.tensor([1.5, 0.0, 0.0]), n - torch.tensor([1.25, 0.0, 0.0])
    nb = Batch({**dict(b.items()), "X": X})
    res = new_ctx(nb).clashscore()
    hx, hm, lp = check_hydrogens(res, nb, what="collinear")
    assert lp[k] == 1 and hm[k, 0] == 0 and new_ctx(b).hydrogens().hmask.reshape(-1, 13)[k, 0] == 1
    assert_same_bytes(words(res), reference(nb, res), "collinear")


def test_the_partner_cap_keeps_the_lowest_codes_and_the_true_count():
    b = O.batch("c64")
    X, am, rt, chain, offs = arrays(b)
    ctx = new_ctx(b)
    radius = A.default_radius(rt, am)
    radius[30, 1] = 6.0                                      # one CA as large as a residue: far more than four partners
    res = ctx.clashscore(radius=torch.from_numpy(radius))
    ref = A.clash(X, res.hxyz.reshape(-1, 13, 3).cpu().numpy(), res.hmask.reshape(-1, 13).cpu().numpy(), radius, rt, chain, offs,
                  res.link_prev.reshape(-1).cpu().numpy())
    got = words(res)
    assert_same_bytes(got, ref, "cap")
    n = int(got["n_clash"][30, 1, 0])
    assert n >= 40 and (np.diff(got["partners"][30, 1]) > 0).all() and got["partners"][30, 1, 0] >= 0
    mine = sorted((j - 0) * 27 + y if (i, x) == (30, 1) else i * 27 + x for i, x, j, y in ref["pairs"] if (30, 1) in ((i, x), (j, y)))
    assert len(mine) == n and got["partners"][30, 1].tolist() == mine[:4]


# ---- bridges and obstacles -----------------------------------------------------------------------------------------------------------------
def test_link_on_2ftl_excludes_the_bridges_and_drops_hg():
    b = O.batch("2FTL")
    X, am, rt, chain, offs = arrays(b)
    ctx = new_ctx(b)
    ds = ctx.disulfides()
    bonds = ds.bonds()
    assert len(bonds) == 9
    link = ds.partner.cpu().numpy()
    free, bound = ctx.clashscore(rotatable="keep"), ctx.clashscore(link=ds, rotatable="keep")
    hx, hm, lp = check_hydrogens(bound, b, link=link, what="2FTL with link")
    hg = A.get_tables()["names"][4].index("HG") - 14
    for a, c in bonds:
        assert hm[a, hg] == 0 and hm[c, hg] == 0 and free.hmask.reshape(-1, 13)[a, hg] == 1
    ref = reference(b, bound, link=link, rotatable="keep")
    assert_same_bytes(words(bound), ref, "link")
    bridge = lambda p: (p[0], p[2]) in bonds and {p[1], p[3]} <= {4, 5}
    fref = reference(b, free, rotatable="keep")
    assert sum(bridge(p) for p in fref["pairs"]) >= 9 and sum(bridge(p) for p in ref["pairs"]) == 0
    assert int(bound.seg[0, 1]) < int(free.seg[0, 1])
    assert_same_bytes(words(ctx.clashscore(link=ds.partner, rotatable="keep")), ref, "link as a tensor")


def _obstacles(b, n=3):
    """Next to ``n`` backbone N atoms: an atom 2.0 A away named polar, one 2.0 A away not polar, one 6 A away."""
    X, am, rt, chain, offs = arrays(b)
    rows = np.nonzero((rt != 14) & (am[:, 0] != 0))[0]
    xyz, pol = [], []
    for r in rows[np.linspace(1, len(rows) - 1, n).astype(int)]:
        xyz += [X[r, 0] + np.float32((2.0, 0, 0)), X[r, 0] + np.float32((0, 2.0, 0)), X[r, 0] + np.float32((0, 0, 6.0))]
        pol += [1, 0, 1]
    return np.array(xyz, np.float32), np.array(pol, np.uint8)


def test_obstacle_atoms_by_hand_and_with_the_batch():
    from packppi_amd.featurize import protein_to_batch
    b = O.batch("c24")
    oxyz, opol = _obstacles(b)
    oxyzr = np.concatenate([oxyz, np.full((len(oxyz), 1), 1.5, np.float32)], 1)
    ctx = new_ctx(b)
    base = words(ctx.clashscore())
    ctx.set_obstacles(torch.from_numpy(oxyzr))
    res = ctx.clashscore(obst_polar=torch.from_numpy(opol))
    ref = reference(b, res, obst=oxyzr, obst_off=[0, len(oxyzr)], obst_polar=opol)
    got = words(res)
    assert_same_bytes(got, ref, "obstacles by hand")
    assert got["seg"][0, 6] >= 6 and np.array_equal(got["partners"], base["partners"]) and np.array_equal(got["n_clash"][..., 0], base["n_clash"][..., 0])
    blind = ctx.clashscore()
    bref = reference(b, blind, obst=oxyzr, obst_off=[0, len(oxyzr)])
    assert_same_bytes(words(blind), bref, "obstacles, none named polar")
    assert bref["seg"][0, 6] >= ref["seg"][0, 6]             # the allowance only ever removes overlaps
    assert float(res.clashscore_obstacles[0]) == 1000.0 * (got["seg"][0, 1] + got["seg"][0, 6]) / got["seg"][0, 0]
    ctx.set_obstacles(None)
    assert_same_bytes(words(ctx.clashscore()), base, "after set_obstacles(None)")
    with pytest.raises(ValueError, match="without obstacle atoms"):
        ctx.clashscore(obst_polar=torch.from_numpy(opol))
    # the batch carries them
    ob = dict(xyz=oxyz, radius=np.full(len(oxyz), 1.5, np.float32), element=["N" if p else "C" for p in opol])
    wb = protein_to_batch(O.protein("c24"), obstacles=ob)
    assert_same_bytes(words(new_ctx(wb).clashscore()), ref, "obstacles of the batch")


# ---- the C entries refuse ------------------------------------------------------------------------------------------------------------------
def test_abi_refusals_leave_the_outputs_untouched():
    from packppi_amd.batch import Batch
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context, _stream, load
    lib = load()
    b = O.batch("c24")
    ctx = new_ctx(b)
    tabs = ctx.allatom_tables()
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)
    st = lambda: _stream(torch.device(DEV))
    hout = [torch.full((24, 13, 3), 77.0, device=DEV), torch.full((24, 13), 77, dtype=torch.uint8, device=DEV),
            torch.full((24,), 77, dtype=torch.uint8, device=DEV)]

    def hyd(h=ctx.handle, p=tabs.place, q=tabs.param, outs=hout):
        return lib.pp_hydrogens(h, None, ptr(p), ptr(q), None, *[ptr(t) for t in outs], st())
    for kw in (dict(h=None), dict(p=None), dict(q=None), dict(outs=[None, hout[1], hout[2]]), dict(outs=[hout[0], None, hout[2]]),
               dict(outs=[hout[0], hout[1], None])):
        assert hyd(**kw) == 1 and b"pp_hydrogens" in lib.pp_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in hout)
    assert hyd() == 0
    good = ctx.hydrogens()
    assert torch.equal(hout[0], good.hxyz.reshape(24, 13, 3)) and torch.equal(hout[1], good.hmask.reshape(24, 13))
    radius = tabs.radius
    out = [torch.full(s, 77, dtype=torch.int32, device=DEV) for s in ((24, 27, 4), (24, 27, 2), (24, 4), (1, 8))]
    op = torch.ones(3, dtype=torch.uint8, device=DEV)

    def cl(h=ctx.handle, hx=hout[0], hm=hout[1], r=radius, a=tabs.acls, s=tabs.aa_sep, lp=hout[2], o=None, cut=0.4, hb=0.6, outs=out):
        return lib.pp_clashscore(h, None, ptr(hx), ptr(hm), ptr(r), ptr(a), ptr(s), ptr(lp), None, ptr(o), cut, hb,
                                 *[ptr(t) for t in outs], st())
    bad = [dict(h=None), dict(hx=None), dict(hm=None), dict(r=None), dict(a=None), dict(s=None), dict(lp=None),
           dict(outs=[out[0], None, out[2], out[3]]), dict(outs=[out[0], out[1], None, out[3]]), dict(outs=[out[0], out[1], out[2], None]),
           dict(cut=float("nan")), dict(cut=float("inf")), dict(hb=-0.1), dict(hb=float("nan")), dict(o=op)]
    for kw in bad:
        assert cl(**kw) == 1 and b"pp_clashscore" in lib.pp_last_error(), kw
    torch.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in out)
    assert cl() == 0
    assert_same_bytes(dict(zip(KEYS, (t.cpu().numpy() for t in out))), words(ctx.clashscore(rotatable="keep")), "after the refusals")
    nb = Batch({k: v for k, v in b.to(DEV).items() if k != "chain_indices"})
    bare = Context(geometry_plan(torch.device(DEV)), nb)
    assert hyd(h=bare.handle) == 1 and b"chain_indices" in lib.pp_last_error()
    assert cl(h=bare.handle) == 1 and b"chain_indices" in lib.pp_last_error()
    with pytest.raises(RuntimeError, match="chain_indices"):
        bare.hydrogens()


def test_a_table_entry_outside_its_range_is_found_on_the_device():
    from packppi_amd import constants as rc
    b = O.batch("c24")
    ctx = new_ctx(b)
    good = ctx.hydrogens()
    assert ctx.saturated() == 0
    place = torch.from_numpy(rc.hydrogen_place.copy())
    rt = b["residue_type"].reshape(-1).numpy()
    t = int(rt[3])
    place[t, 1, 2] = 15                                      # a neighbour slot that does not exist
    place[t, 2, 0] = 9                                       # a kind that does not exist
    h = ctx.hydrogens(place=place, param=torch.from_numpy(rc.hydrogen_param))
    assert ctx.saturated() == 8
    hm, gm = h.hmask.reshape(-1, 13).cpu().numpy(), good.hmask.reshape(-1, 13).cpu().numpy()
    hit = rt == t
    assert (hm[hit][:, 1:3] == 0).all() and (gm[hit][:, 1] == 1).all()
    keep = np.ones_like(hm, bool)
    keep[hit, 1:3] = False
    assert np.array_equal(hm[keep], gm[keep]) and torch.equal(h.hxyz.reshape(-1, 13, 3)[torch.from_numpy(keep)], good.hxyz.reshape(-1, 13, 3)[torch.from_numpy(keep)])


# ---- ensembles and the command lines ---------------------------------------------------------------------------------------------------------
def test_sample_ensemble_columns_against_a_call_per_decoy(weights):
    """Seeded random weights and the 4-point schedule of tests/test_ensemble_gpu.py."""
    from packppi_amd.module import TDiffusionModule
    model = TDiffusionModule(weights, device=DEV)
    model.schedule = torch.linspace(1, 0, 4)
    b = O.batch("c64").to(DEV)
    plain = model.sample_ensemble(b, 3, seed=11, return_all=True)
    assert not {"clashscore", "clashes_interface"} & set(plain)
    out = model.sample_ensemble(b, 3, seed=11, return_all=True, clashscore=True)
    chi, packed = out["decoys"]
    assert torch.equal(chi, plain["decoys"][0]) and torch.equal(out["selected"], plain["selected"])
    assert out["clashscore"].dtype == torch.float64 and tuple(out["clashscore"].shape) == (3,) and out["clashes_interface"].dtype == torch.int32
    ctx = new_ctx(O.batch("c64"))
    for d in range(3):
        res = ctx.clashscore(chi=chi[:, 64 * d:64 * d + 64])
        assert float(out["clashscore"][d]) == float(res.clashscore[0]) and int(out["clashes_interface"][d]) == int(res.seg[0, 2])
    assert len({float(v) for v in out["clashscore"]}) == 3 and float(out["clashscore"].min()) > 0


def _same_files_plus(plain, flagged, extra):
    """Every file of ``plain`` is in ``flagged`` with the same bytes, and ``flagged`` has exactly the ``extra`` names more."""
    a, b = {p.name for p in plain.iterdir()}, {p.name for p in flagged.iterdir()}
    assert b - a == set(extra) and a <= b, (sorted(a), sorted(b))
    return [n for n in sorted(a) if (plain / n).read_bytes() != (flagged / n).read_bytes()]


def test_eval_diffusion_with_and_without_the_flags(tmp_path, capsys):
    from packppi_amd import synth
    from packppi_amd.analysis import CLASHES_CSV_HEADER, clashes_csv_text
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    src = str(tmp_path / "in.pdb")
    with open(src, "w") as fh:
        fh.write(to_pdb(synth.make_complex(64, 11)))
    base = ["--input", src, "--molprobity_clash_loc", "none", "--random_weights", "0", "--seed", "7", "--steps", "3", "--device", DEV]
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    eval_diffusion.main(base + ["--outdir", str(plain)])
    assert "clashscore (all atoms" not in capsys.readouterr().out
    eval_diffusion.main(base + ["--outdir", str(flagged), "--clashscore", "--hydrogens"])
    text = capsys.readouterr().out
    assert _same_files_plus(plain, flagged, ["clashes.csv", "structure_H.pdb"]) == []
    protein = from_pdb_file(src)
    b = protein_to_batch(protein).to(DEV)
    args = eval_diffusion.parse_args(base + ["--outdir", str(tmp_path / "again")])
    chi = eval_diffusion.load_model(args).sampling(b, seed=7)
    ctx = new_ctx(b)
    res, native = ctx.clashscore(chi=chi), ctx.clashscore()
    want = clashes_csv_text(protein, res.xyz[0].cpu().numpy(), res.hxyz[0].cpu().numpy(), res.partners[0].cpu().numpy(),
                            res.radius.reshape(-1, 27).cpu().numpy(), 0.6, native.partners[0].cpu().numpy())
    got = (flagged / "clashes.csv").read_text()
    assert got == want and got.startswith(CLASHES_CSV_HEADER + "\n")
    status = [ln.rsplit(",", 1)[1] for ln in got.splitlines()[1:]]
    assert set(status) <= {"kept", "gained", "lost"} and "kept" in status and "gained" in status
    seg = res.seg[0].tolist()
    assert (f"clashscore (all atoms, placed hydrogens; not MolProbity): {float(res.clashscore[0]):.2f}, {seg[1]} serious overlaps, "
            f"{seg[2]} between chains, {seg[7]} backbone only; the input's own side chains: {float(native.clashscore[0]):.2f}") in text
    # structure_H.pdb: the heavy atoms of structure.pdb bit for bit, and as many hydrogens as the device placed
    a, c = from_pdb_file(flagged / "structure_H.pdb"), from_pdb_file(flagged / "structure.pdb")
    assert all(a[k].tobytes() == c[k].tobytes() for k in c)
    n_h = sum(ln.startswith("ATOM") and ln[76:78].strip() == "H" for ln in (flagged / "structure_H.pdb").read_text().splitlines())
    assert n_h == int(res.hmask.sum())
    # decoys: ensemble.csv gains the two columns, every other file is as without the flag
    e0, e1 = tmp_path / "ens0", tmp_path / "ens1"
    eval_diffusion.main(base + ["--outdir", str(e0), "--n_decoys", "2"])
    eval_diffusion.main(base + ["--outdir", str(e1), "--n_decoys", "2", "--clashscore"])
    assert _same_files_plus(e0, e1, ["clashes.csv"]) == ["ensemble.csv"]
    r0 = [ln.split(",") for ln in (e0 / "ensemble.csv").read_text().strip().split("\n")]
    r1 = [ln.split(",") for ln in (e1 / "ensemble.csv").read_text().strip().split("\n")]
    assert r1[0] == r0[0] + ["clashscore", "clashes_interface"] and [r[:-2] for r in r1] == r0 and len(r1) == 3
    assert all(float(r[-2]) > 0 and int(r[-1]) >= 0 for r in r1[1:])


def test_eval_diffusion_hands_the_bridges_on(tmp_path):
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.pdb_io import to_pdb
    src = tmp_path / "2ftl.pdb"
    src.write_text(to_pdb(O.protein("2FTL")))
    out = tmp_path / "out"
    eval_diffusion.main(["--input", str(src), "--molprobity_clash_loc", "none", "--random_weights", "0", "--seed", "7", "--steps", "3",
                         "--device", DEV, "--outdir", str(out), "--disulfides", "auto", "--clashscore", "--hydrogens"])
    text = (out / "structure_H.pdb").read_text()
    assert text.startswith("SSBOND") and text.count("SSBOND") == 9
    hg = [ln for ln in text.splitlines() if ln.startswith("ATOM") and ln[17:20] == "CYS" and ln[12:16].strip() == "HG"]
    cys = {ln[21:26] for ln in text.splitlines() if ln.startswith("ATOM") and ln[17:20] == "CYS"}
    assert len(hg) == len(cys) - 18
    rows = [ln.split(",") for ln in (out / "clashes.csv").read_text().splitlines()[1:]]
    assert not [r for r in rows if r[3] == r[7] == "SG" and float(r[8]) < 2.5]             # a closed bridge is no overlap


def test_mutate_and_proximal_optimize_with_and_without_the_flags(tmp_path, capsys):
    from packppi_amd.analysis import CLASHES_CSV_HEADER
    from packppi_amd.cli import mutate, proximal_optimize
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    pdb = tmp_path / "1brs.pdb"
    pdb.write_text(to_pdb(O.protein("1BRS")))
    base = ["--input", str(pdb), "--mutstr", "LA87F", "--device", "cuda", "--random_weights", "3", "--steps", "3", "--seed", "7",
            "--n_decoys", "2"]
    m0, m1 = tmp_path / "m0", tmp_path / "m1"
    mutate.main(base + ["--outdir", str(m0)])
    mutate.main(base + ["--outdir", str(m1), "--clashscore", "--hydrogens"])
    assert _same_files_plus(m0, m1, ["clashes_LA87F.csv", "mutant_LA87F_H.pdb"]) == ["mutants.csv"]
    r0 = [ln.split(",") for ln in (m0 / "mutants.csv").read_text().splitlines()]
    r1 = [ln.split(",") for ln in (m1 / "mutants.csv").read_text().splitlines()]
    assert r1[0] == r0[0] + ["clashscore", "clashes_interface"] and [r[:-2] for r in r1] == r0 and float(r1[1][-2]) > 0
    assert (m1 / "clashes_LA87F.csv").read_text().startswith(CLASHES_CSV_HEADER + "\n")
    a, c = from_pdb_file(m1 / "mutant_LA87F_H.pdb"), from_pdb_file(m1 / "mutant_LA87F.pdb")
    assert all(a[k].tobytes() == c[k].tobytes() for k in c)
    assert " HZ  PHE A  87" in (m1 / "mutant_LA87F_H.pdb").read_text()                    # the mutant's hydrogens, not the wild type's
    capsys.readouterr()
    pbase = ["--input", str(pdb), "--molprobity_clash_loc", "none", "--num_steps", "5", "--device", "cuda"]
    p0, p1 = tmp_path / "p0", tmp_path / "p1"
    proximal_optimize.main(pbase + ["--outdir", str(p0)])
    assert "clashscore (all atoms" not in capsys.readouterr().out
    proximal_optimize.main(pbase + ["--outdir", str(p1), "--clashscore", "--hydrogens"])
    assert "the input's own side chains: " in capsys.readouterr().out
    assert _same_files_plus(p0, p1, ["clashes.csv", "structure_H.pdb"]) == []
    status = {ln.rsplit(",", 1)[1] for ln in (p1 / "clashes.csv").read_text().splitlines()[1:]}
    assert "kept" in status and status <= {"kept", "gained", "lost"}


def test_protein_analysis_reports_the_device_score_only_when_asked(tmp_path):
    from packppi_amd.analysis import ProteinAnalysis
    from packppi_amd.pdb_io import to_pdb
    pdb = tmp_path / "1brs.pdb"
    pdb.write_text(to_pdb(O.protein("1BRS")))
    plain = ProteinAnalysis("none", str(tmp_path / "a"), DEV).get_metric(str(pdb), str(pdb))
    asked = ProteinAnalysis("none", str(tmp_path / "b"), DEV, device_clashscore=True).get_metric(str(pdb), str(pdb))
    assert "clashscore_device" not in plain and plain["clashscore"] is None and asked["clashscore"] is None
    assert set(asked) == set(plain) | {"clashscore_device"}
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file
    want = float(new_ctx(protein_to_batch(from_pdb_file(pdb))).clashscore().clashscore[0])   # the file's three decimals
    assert abs(asked["clashscore_device"] - want) <= 1e-9 and 15.0 < want < 30.0            # the fixture itself: 62 of 2998 atoms, 20.7


def test_functional_entries():
    from packppi_amd.functional import add_hydrogens, clashscore
    b = O.batch("c24").to(DEV)
    ctx = new_ctx(O.batch("c24"))
    chi = torch.zeros(1, 24, 4, device=DEV)
    assert torch.equal(add_hydrogens(b, chi).hxyz, ctx.hydrogens(chi=chi).hxyz)
    assert_same_bytes(words(clashscore(b, chi)), words(ctx.clashscore(chi=chi)), "functional")
    assert_same_bytes(words(clashscore(b)), words(ctx.clashscore()), "functional at X")
