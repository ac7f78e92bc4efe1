"""Solvent-accessible surface on the device, through the C ABI (pp_sasa).

Reference: the NumPy restatement of tests/test_sasa_host.py (brute force over all atoms of a segment).  counts must have the BYTES of
its float32 form and must equal its float64 form at every point that is not ambiguous (an occluder with |d2 - R_b^2| < 1e-4 A^2 in
float64; at most 0.1 % of a case's points may be).  area: within 2e-6 relative of the float64 sum over the same counts -- three
roundings per term and at most 13 additions stay below 16 x 2^-24 = 9.5e-7; kf and R_a, rounded once each, add 3 x 2^-24.  Nothing
measured on the device enters a bound."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from . import test_sasa_host as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
AREA_RTOL = 2e-6


def new_ctx(batch, obstacles=None, ranges=None):
    """A fresh geometry context of ``batch`` (moved to the device; the context keeps it alive), optionally with obstacles."""
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    gb = batch.to(DEV)
    ctx = Context(geometry_plan(torch.device(DEV)), gb)
    ctx._keep = gb
    if obstacles is not None:
        ctx.set_obstacles(torch.as_tensor(obstacles), ranges)
    return ctx


def points(P):
    from packppi_amd.analysis import sphere_points
    return sphere_points(P)


def device_counts(ctx, **kw):
    res = ctx.sasa(want_counts=True, **kw)
    return res.counts.reshape(-1, 14, 4).cpu().numpy(), res


# ---- the cases and their references (computed once) ---------------------------------------------------------------------------------------
def _pack3():
    from packppi_amd.batch import pack
    return pack([H.make(97, 267), H.make(65, 9), H.make(97, 267)])


def _damaged64():
    """A complex with incomplete side chains (synth.drop_atoms): missing atoms have radius 0 and a zeroed coordinate in X, one row has
    no atom at all (a backbone atom is missing), others only their backbone."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    return protein_to_batch(synth.drop_atoms(synth.make_complex(64, 11), 64))


def _pack3_damaged():
    from packppi_amd.batch import pack
    return pack([H.make(97, 267), _damaged64(), H.make(97, 267)])


def _padded():
    from packppi_amd import synth
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_data
    return collate([protein_to_data(synth.make_complex(40, 2)), protein_to_data(synth.make_complex(36, 3))])


CASES = {
    "c24": lambda: H.make(24, 5), "c64": lambda: H.make(64, 11), "c97": lambda: H.make(97, 267),
    "three_chains": lambda: H.make(45, 3, n_chains=3),
    "c24_row_off": lambda: H.make(24, 5, zero_row=7), "c64_row_off": lambda: H.make(64, 11, zero_row=0),
    "c97_row_off": lambda: H.make(97, 267, zero_row=96), "three_chains_row_off": lambda: H.make(45, 3, n_chains=3, zero_row=20),
    "c65": lambda: H.make(65, 9), "pack3": _pack3, "padded": _padded,
    "damaged64": _damaged64, "pack3_damaged": _pack3_damaged,
}
PACKS = {"pack3": ("c97", "c65", "c97"), "pack3_damaged": ("c97", "damaged64", "c97")}


@functools.lru_cache(maxsize=None)
def case(name):
    b = CASES[name]()
    return b, H.arrays(b), H.seg_table(b)


def reference(name, P=96, probe=1.4, fp64=True):
    """(counts of the fp32 restatement, counts of the fp64 one, its ambiguous points) of a case, computed once."""
    return _reference(name, P, probe, fp64)


@functools.lru_cache(maxsize=None)
def _reference(name, P, probe, fp64):
    b, (X, radius, chain), offs = case(name)
    if name in PACKS:
        # the restatement works segment by segment: on the same rows it is the references of the three complexes, back to back
        parts = PACKS[name]
        assert all(np.array_equal(np.concatenate([case(p)[1][k] for p in parts]), (X, radius, chain)[k], equal_nan=(k == 0)) for k in range(3))
        assert offs == {"pack3": [0, 97, 162, 259], "pack3_damaged": [0, 97, 161, 258]}[name]
        return tuple(np.concatenate([reference(p, P, probe, fp64)[k] for p in parts]) for k in range(3))
    c32 = H.restate(X, radius, chain, offs, points(P), probe)
    c64, amb = H.restate(X, radius, chain, offs, points(P), probe, dtype=np.float64, want_ambiguous=True) if fp64 else (None, None)
    return c32, c64, amb


# ---- 1, 2. bytes of the fp32 restatement, the fp64 restatement outside ambiguous points, areas ---------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_counts_and_areas_against_the_restatement(name):
    b, (X, radius, chain), offs = case(name)
    c32, c64, amb = reference(name)
    got, res = device_counts(new_ctx(b))
    frac = amb[radius > 0].mean()
    clear = ~amb.any(-1)
    print(f"{name}: {int((radius > 0).sum())} atoms in {len(offs) - 1} segment(s), ambiguous points {frac:.2e}, words that differ from "
          f"fp32 {(got != c32).sum()}, from fp64 outside ambiguous points {(got[clear] != c64[clear]).sum()}")
    assert got.dtype == np.int32 and got.tobytes() == c32.tobytes()
    assert frac <= 1e-3
    assert np.array_equal(got[clear], c64[clear])
    assert (np.diff(got, axis=-1) <= 0).all() and np.array_equal(got[..., 3], got[..., 2])       # no obstacles: level 3 = level 2
    want = H.area_fp64(got, radius, 1.4, 96)
    area = res.area.reshape(-1, 4).cpu().double().numpy()
    assert (np.abs(area - want) <= AREA_RTOL * np.abs(want)).all()
    seg = res.seg_area.cpu().numpy()
    assert seg.dtype == np.float64 and seg.shape == (len(offs) - 1, 4)
    for s, (lo, hi) in enumerate(zip(offs[:-1], offs[1:])):
        ref = res.area.reshape(-1, 4)[lo:hi].cpu().double().numpy().sum(0)
        assert np.allclose(seg[s], ref, rtol=1e-12, atol=0)
    # a row without atoms gives zeros
    empty = ~(radius > 0).any(1)
    assert (got[empty] == 0).all() and (area[empty] == 0).all()
    if name.endswith("row_off") or "damaged" in name:
        assert empty.any()
    if "damaged" in name:
        # a missing atom sits at the origin of X with radius 0: it has no points and buries nobody's
        am = b["atom_mask"].reshape(-1, 14).numpy()
        table = H.rc.atom14_mask[b["residue_type"].reshape(-1).numpy()]
        gone = (table > 0) & (am == 0)
        assert gone.sum() >= 20 and (X[gone] == 0).all() and (got[gone] == 0).all()
        assert ((am[:, 4:].sum(1) == 0) & (am[:, :4].sum(1) == 4) & (table[:, 4] > 0)).sum() >= 2       # backbone-only rows
    # the derived quantities are what they say
    per_row = torch.from_numpy(got.sum(1))
    assert torch.equal(res.interface.reshape(-1).cpu(), per_row[:, 1] - per_row[:, 2] > 0)
    assert torch.equal(res.bsa, res.area[..., 1] - res.area[..., 2]) and not bool(res.pocket.any())
    if name in ("c64", "c97", "three_chains"):
        assert bool(res.interface.any()) and float(seg[0, 1] - seg[0, 2]) > 50.0


def test_a_cross_segment_leak_would_show():
    """The outer segments of the pack are the same complex: equal bits, and the bits of the complex alone."""
    b, _, offs = case("pack3")
    got, res = device_counts(new_ctx(b))
    alone, res1 = device_counts(new_ctx(case("c97")[0]))
    assert np.array_equal(got[:97], alone) and np.array_equal(got[162:], alone)
    assert torch.equal(res.area[0, :97], res1.area[0]) and torch.equal(res.area[0, 162:], res1.area[0])
    assert torch.equal(res.seg_area[0], res1.seg_area[0]) and torch.equal(res.seg_area[2], res1.seg_area[0])
    mid, _ = device_counts(new_ctx(case("c65")[0]))
    assert np.array_equal(got[97:162], mid)


# ---- 3. points and probe --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 96, 250])
@pytest.mark.parametrize("probe", [0.0, 1.4])
def test_point_counts_and_probes(P, probe):
    b, (X, radius, chain), offs = case("c24")
    c32, _, _ = reference("c24", P, probe, fp64=False)
    got, res = device_counts(new_ctx(b), n_points=P, probe=probe)
    assert got.tobytes() == c32.tobytes() and got.max() <= P
    want = H.area_fp64(got, radius, probe, P)
    area = res.area.reshape(-1, 4).cpu().double().numpy()
    assert (np.abs(area - want) <= AREA_RTOL * np.abs(want)).all()


def test_the_larger_instance_on_a_complex_with_more_than_one_pass():
    """P = 250 takes the 14-items-per-lane instance; 97 rows and an odd row count."""
    b, (X, radius, chain), offs = case("c97")
    c32, _, _ = reference("c97", 250, 1.4, fp64=False)
    got, _ = device_counts(new_ctx(b), n_points=250)
    assert got.tobytes() == c32.tobytes()


# ---- 4. the list is worked off and refilled -------------------------------------------------------------------------------------------------
def test_list_drain():
    b = H.make(160, 31)
    X, radius, chain = H.arrays(b)
    n_atoms = int((radius > 0).sum())
    assert n_atoms == 1167 and n_atoms > H.LIST_CAP
    # with probe 6 the rows inside a row's reach (|CA_i - CA_j| <= rad_i + rad_j + Rmax_i + Rmax_j) hold more atoms than the list
    ca = X[:, 1].astype(np.float64)
    dist = np.where(radius > 0, np.linalg.norm(X.astype(np.float64) - ca[:, None], axis=-1), 0.0)
    rad, rmax = dist.max(1), radius.max(1) + 6.0
    reach = np.linalg.norm(ca[:, None] - ca[None], axis=-1) <= rad[:, None] + rad[None] + rmax[:, None] + rmax[None]
    in_reach = (reach * (radius > 0).sum(1)[None, :]).sum(1)
    assert in_reach.max() > H.LIST_CAP
    c32 = H.restate(X, radius, chain, [0, 160], points(96), 6.0)
    got, _ = device_counts(new_ctx(b), probe=6.0)
    print(f"list drain: {n_atoms} atoms against a list of {H.LIST_CAP}; exposed points left {int(got[..., 2].sum())}")
    assert got.tobytes() == c32.tobytes() and got[..., 2].sum() > 0


# ---- 5. a chain as obstacles ----------------------------------------------------------------------------------------------------------------
def test_chain_as_obstacles_is_the_complex():
    from packppi_amd.batch import TENSOR_KEYS, Batch
    full = case("c64")[0]
    X, radius, chain = H.arrays(full)
    rows_a = np.nonzero(chain == chain[0])[0]
    rows_b = np.nonzero(chain != chain[0])[0]
    part = Batch(num_proteins=1, max_size=len(rows_a))
    for k in TENSOR_KEYS:
        part[k] = full[k][:, torch.from_numpy(rows_a)]
    keep = radius[rows_b] > 0
    ob = np.concatenate([X[rows_b][keep], radius[rows_b][keep][:, None]], 1).astype(np.float32)
    whole, _ = device_counts(new_ctx(full))
    ctx = new_ctx(part, ob)
    got, res = device_counts(ctx)
    assert np.array_equal(got[..., 3], whole[rows_a][..., 2])                        # exact integers
    assert np.array_equal(got[..., :2], whole[rows_a][..., :2]) and np.array_equal(got[..., 2], got[..., 1])
    assert bool(res.pocket.any()) and not bool(res.interface.any())
    assert torch.equal(res.pocket.reshape(-1).cpu(), torch.from_numpy((whole[rows_a].sum(1)[:, 1] - whole[rows_a].sum(1)[:, 2]) > 0))
    ctx.set_obstacles(None)
    cleared, res0 = device_counts(ctx)
    assert np.array_equal(cleared[..., 3], cleared[..., 2]) and np.array_equal(cleared[..., :3], got[..., :3])
    assert not bool(res0.pocket.any())


def test_obstacle_drain():
    """1500 obstacle atoms inside one row's reach (more than the list holds), 40 far away, some with radius 0."""
    b, (X, radius, chain), offs = case("c24")
    g = np.random.default_rng(12)
    K = 9
    u = g.normal(size=(1500, 3))
    near = X[K, 1] + u / np.linalg.norm(u, axis=1, keepdims=True) * (g.uniform(0, 1, (1500, 1)) ** (1 / 3) * 9.0)
    far = X[K, 1] + 300.0 + g.uniform(0, 30, (40, 3))
    ob = np.concatenate([np.concatenate([near, far]), g.choice([1.7, 1.55, 1.52, 1.8, 0.0], size=(1540, 1))], 1).astype(np.float32)
    ob = ob[g.permutation(1540)]
    assert (ob[:, 3] > 0).sum() > H.LIST_CAP
    c32 = H.restate(X, radius, chain, offs, points(96), 1.4, ob)
    got, res = device_counts(new_ctx(b, ob))
    assert got.tobytes() == c32.tobytes()
    assert (got[K, :, 3] < got[K, :, 2]).any() and bool(res.pocket[0, K])
    # a range per segment is honoured: the first 300 atoms only
    c300 = H.restate(X, radius, chain, offs, points(96), 1.4, ob, ranges=[(0, 300)])
    got300, _ = device_counts(new_ctx(b, ob, [(0, 300)]))
    assert got300.tobytes() == c300.tobytes() and not np.array_equal(got300, got)


# ---- 6. packing, decoys, reproducibility ----------------------------------------------------------------------------------------------------
def test_decoys_get_the_bits_of_their_own_run():
    from packppi_amd.batch import replicate
    b = case("c64")[0]
    D, n = 3, 64
    g = torch.Generator().manual_seed(20)
    chis = ((torch.rand(D, n, 4, generator=g) * 2 - 1) * np.pi) * b.SC_D_mask
    ctx = new_ctx(replicate(b, D))
    chi = chis.reshape(1, D * n, 4)
    got, res = device_counts(ctx, chi=chi)
    again, res2 = device_counts(ctx, chi=chi)
    assert np.array_equal(got, again) and torch.equal(res.area, res2.area) and torch.equal(res.seg_area, res2.seg_area)
    solo = new_ctx(b)
    for d in range(D):
        one, r1 = device_counts(solo, chi=chis[d:d + 1])
        assert np.array_equal(got[d * n:(d + 1) * n], one)
        assert torch.equal(res.area[0, d * n:(d + 1) * n], r1.area[0]) and torch.equal(res.seg_area[d], r1.seg_area[0])
    assert not np.array_equal(got[:n], got[n:2 * n])                                 # the decoys differ
    # xyz= is the same call on given coordinates; the functional form uses the geometry plan
    from packppi_amd.functional import solvent_accessibility
    gb = b.to(DEV)
    via_xyz, _ = device_counts(solo, xyz=solo.atom14(chis[0:1]))
    assert np.array_equal(via_xyz, got[:n])
    f = solvent_accessibility(gb, chis[0:1].to(DEV), want_counts=True)
    assert np.array_equal(f.counts.reshape(-1, 14, 4).cpu().numpy(), got[:n])


def test_packed_with_obstacles_in_front_and_behind():
    from packppi_amd.batch import Batch, pack
    a = Batch(case("c64")[0])                             # complexes shorter than 32 rows cannot share a packed context
    ob = torch.from_numpy(H.ligand_near(a, 12, 11))
    a["obstacle_xyzr"], a["obstacle_offsets"], a["obstacle_offsets_host"] = ob, torch.tensor([0, 12], dtype=torch.int32), [0, 12]
    other = case("three_chains")[0]
    alone, _ = device_counts(new_ctx(a))
    alone_o, _ = device_counts(new_ctx(other))
    assert (alone[..., 3] < alone[..., 2]).any()
    for order in ((a, other), (other, a)):
        got, _ = device_counts(new_ctx(pack(order)))
        lo = 0
        for c in order:
            n = c.X.shape[1]
            assert np.array_equal(got[lo:lo + n], alone if c is a else alone_o)
            lo += n


# ---- 7. NaN -----------------------------------------------------------------------------------------------------------------------------------
def test_a_nan_coordinate_is_never_buried_and_buries_nothing():
    from packppi_amd.batch import Batch
    b = Batch(case("c24")[0])
    b["X"] = b["X"].clone()
    X0, radius, chain = H.arrays(b)
    row, slot = 11, int(np.nonzero(radius[11] > 0)[0][-1])
    b["X"][0, row, slot, 1] = float("nan")
    X = H.arrays(b)[0]
    c32 = H.restate(X, radius, chain, [0, 24], points(96), 1.4)
    got, res = device_counts(new_ctx(b))
    assert got.tobytes() == c32.tobytes()
    assert (got[row, slot] == 96).all()
    clean = reference("c24")[0]
    assert (got >= clean)[np.arange(24) != row].all() and (got > clean).any()          # its neighbours lost an occluder


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_of_the_c_entry():
    from packppi_amd import lib as L
    from packppi_amd.batch import Batch
    b = case("c24")[0]
    ctx = new_ctx(b)
    l, s = L.load(), L._stream(torch.device(DEV))
    radius = torch.from_numpy(H.arrays(b)[1]).to(DEV)
    pts = torch.from_numpy(points(96)).to(DEV)
    area = torch.full((24, 4), -1.0, device=DEV)
    call = lambda h, r, p, n, probe, a: l.pp_sasa(h, None, L._ptr(r), L._ptr(p), n, probe, None, L._ptr(a), None, s)
    assert call(ctx.handle, radius, pts, 96, 1.4, area) == 0
    assert float(area.min()) >= 0.0
    assert call(None, radius, pts, 96, 1.4, area) == 1
    assert call(ctx.handle, None, pts, 96, 1.4, area) == 1 and call(ctx.handle, radius, None, 96, 1.4, area) == 1
    assert call(ctx.handle, radius, pts, 96, 1.4, None) == 1 and b"null" in l.pp_last_error()
    for n in (0, -3, H.MAX_POINTS + 1):
        assert call(ctx.handle, radius, pts, n, 1.4, area) == 1 and b"n_points" in l.pp_last_error()
    for probe in (-0.5, float("nan"), float("inf")):
        assert call(ctx.handle, radius, pts, 96, probe, area) == 1 and b"probe" in l.pp_last_error()
    bare = new_ctx(Batch(X=b.X, residue_type=b.residue_type, BB_D=b.BB_D, atom_mask=b.atom_mask))
    assert call(bare.handle, radius, pts, 96, 1.4, area) == 1 and b"chain_indices" in l.pp_last_error()
    with pytest.raises(RuntimeError):
        bare.sasa()
    with pytest.raises(RuntimeError, match="n_points"):
        ctx.sasa(n_points=257)
    with pytest.raises(RuntimeError, match="probe"):
        ctx.sasa(probe=-1.0)
    with pytest.raises(ValueError):
        ctx.sasa(xyz=torch.zeros(3, 14, 3))


# ---- 9. command line ----------------------------------------------------------------------------------------------------------------------------
def test_eval_diffusion_with_the_flag(tmp_path):
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.pdb_io import from_pdb_file, insert_obstacle_lines, obstacle_atoms, to_pdb
    from .test_obstacles_host import _rec
    prot = synth.make_complex(48, 5)
    lig = H.ligand_near(protein_to_batch(prot), 9, 3)
    het = [_rec("HETATM", 900 + k, f" C{k + 1} ", " ", "LIG", "A", 301, float(q[0]), float(q[1]), float(q[2]), 1.0, "C") for k, q in enumerate(lig)]
    src = str(tmp_path / "in.pdb")
    with open(src, "w") as fh:
        fh.write(insert_obstacle_lines(to_pdb(prot), het))
    base = ["--input", src, "--molprobity_clash_loc", "none", "--random_weights", "0", "--seed", "7", "--steps", "3", "--device", DEV]
    with pytest.raises(SystemExit):
        eval_diffusion.main(base + ["--outdir", str(tmp_path / "no"), "--repack", "pocket"])
    out = tmp_path / "out"
    eval_diffusion.main(base + ["--outdir", str(out), "--sasa", "--n_decoys", "2", "--obstacles", "hetero"])
    for name in ("sasa.csv", "ensemble.csv", "structure.pdb", "decoy_000.pdb", "decoy_001.pdb", "obstacles.csv"):
        assert (out / name).exists(), name
    rows = [ln.split(",") for ln in (out / "ensemble.csv").read_text().strip().split("\n")]
    assert rows[0] == ["decoy", "key", "dev", "clash", "selected", "bsa"] and len(rows) == 3
    # the seeded run again, in process: the same decoys, so the same column
    protein = from_pdb_file(src)
    b = protein_to_batch(protein, obstacles=obstacle_atoms(src)).to(DEV)
    assert b.obstacle_xyzr.shape[0] == 9
    args = eval_diffusion.parse_args(base + ["--outdir", str(tmp_path / "again"), "--obstacles", "hetero"])
    ens = eval_diffusion.load_model(args).sample_ensemble(b, 2, seed=7, return_all=True)
    chi, packed = ens["decoys"]
    assert "bsa" not in ens
    seg = new_ctx(packed).sasa(chi=chi).seg_area.cpu().numpy()
    assert [float(r[5]) for r in rows[1:]] == [float(seg[d, 1] - seg[d, 2]) for d in range(2)]
    best = [int(r[4]) for r in rows[1:]].index(1)
    # sasa.csv is the selected decoy's
    n = packed.seg_offsets_host[1]
    res = new_ctx(b).sasa(chi=chi[:, best * n:(best + 1) * n])
    table = [ln.split(",") for ln in (out / "sasa.csv").read_text().strip().split("\n")]
    assert ",".join(table[0]) == "chain,number,name,sasa_residue,sasa_chain,sasa_complex,sasa_ligand,bsa,exposure" and len(table) == 49
    assert [r[0] for r in table[1:]] == list(protein["chain_id"]) and [int(r[1]) for r in table[1:]] == [int(x) for x in protein["residue_index"]]
    assert [r[3:7] for r in table[1:]] == [[f"{v:.3f}" for v in row] for row in res.area[0].cpu().tolist()]
    # the new selectors, on the device: the pocket rows are those the ligand buries
    from packppi_amd.selection import sasa_selection
    pocket = sasa_selection(b, "pocket")
    inter = sasa_selection(b, "interface")
    assert pocket.any() and inter.any() and pocket.shape == (48,)
    X, radius, chain = H.arrays(b)
    c32 = H.restate(X, radius, chain, [0, 48], points(96), 1.4, b.obstacle_xyzr.cpu().numpy())
    assert np.array_equal(pocket, (c32.sum(1)[:, 2] - c32.sum(1)[:, 3]) > 0) and np.array_equal(inter, (c32.sum(1)[:, 1] - c32.sum(1)[:, 2]) > 0)
    # and through the flag: a pinned run on those rows
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "pk"), "--repack", "pocket", "--obstacles", "hetero"])
    assert (tmp_path / "pk" / "structure.pdb").exists() and not (tmp_path / "pk" / "sasa.csv").exists()
