"""Solvent-accessible surface (pp_sasa) on the CPU: the NumPy restatement that tests/test_sasa_gpu.py compares
the device with, and the host-side surfaces (test points, selectors, sasa.csv).

The restatement is brute force over all atoms of a segment -- no bounding spheres, no lists.  Its float32 form follows the
operation order of include/packppi_hip.h (NumPy rounds every float32 operation on its own); its float64 form is the arbiter: where
the two disagree the point must be AMBIGUOUS (an occluder whose |d2 - R_b^2| is below 1e-4 A^2 in float64)."""
import os
import re

import numpy as np
import pytest

from packppi_amd import constants as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AMBIGUOUS = 1e-4                                 # A^2
HEADER = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
LIST_CAP = int(re.search(r"#define PP_SASA_LIST_CAP (\d+)", HEADER).group(1))
MAX_POINTS = int(re.search(r"#define PP_SASA_MAX_POINTS (\d+)", HEADER).group(1))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def restate(xyz, radius, chain, seg_offs, points, probe, obstacles=None, ranges=None, dtype=np.float32, want_ambiguous=False):
    """counts int32 [N, 14, 4] of the definition (with ``want_ambiguous`` also bool [N, 14, P]: the point has an occluder with
    |d2 - R_b^2| < AMBIGUOUS).  ``xyz`` [N, 14, 3], ``radius`` [N, 14] (present iff > 0), ``chain`` [N], ``seg_offs`` the segment
    table, ``points`` [P, 3], ``obstacles`` [M, 4] with ``ranges`` one (first, count) per segment (default: all of them)."""
    f = dtype
    xyz, radius, pts = np.asarray(xyz, f), np.asarray(radius, f), np.asarray(points, f)
    chain = np.asarray(chain)
    N, P = xyz.shape[0], pts.shape[0]
    probe = f(probe)
    counts = np.zeros((N, 14, 4), np.int32)
    amb = np.zeros((N, 14, P), bool)
    present = radius > 0
    with np.errstate(invalid="ignore", over="ignore"):
        for s in range(len(seg_offs) - 1):
            lo, hi = int(seg_offs[s]), int(seg_offs[s + 1])
            rows, slots = np.nonzero(present[lo:hi])
            rows = rows + lo
            pb = xyz[rows, slots]                                    # [M, 3] the protein occluders of the segment
            Rb = radius[rows, slots] + probe
            cls_chain = chain[rows]
            ob = np.zeros((0, 4), f)
            if obstacles is not None:
                first, count = ranges[s] if ranges is not None else (0, len(obstacles))
                ob = np.asarray(obstacles, f)[first:first + count]
                ob = ob[ob[:, 3] > 0]
            occ = np.concatenate([pb, ob[:, :3]])
            Rocc = np.concatenate([Rb, ob[:, 3] + probe])
            R2 = Rocc * Rocc
            for i in range(lo, hi):
                mine = np.nonzero(present[i])[0]
                if not len(mine):
                    continue
                Ra = radius[i, mine] + probe
                q = xyz[i, mine][:, None, :] + (Ra[:, None, None] * pts[None, :, :])              # [na, P, 3]
                d = q[:, :, None, :] - occ[None, None, :, :]
                dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
                d2 = ((dx * dx) + (dy * dy)) + (dz * dz)                                          # [na, P, M + Mo]
                cls = np.where(rows == i, 0, np.where(cls_chain == chain[i], 1, 2))
                cls = np.concatenate([cls, np.full(len(ob), 3)])[None, :].repeat(len(mine), 0)      # [na, M + Mo]
                itself = np.concatenate([(rows[None, :] == i) & (slots[None, :] == mine[:, None]), np.zeros((len(mine), len(ob)), bool)], 1)
                buried = (d2 < R2[None, None, :]) & ~itself[:, None, :]
                m = np.where(buried, cls[:, None, :], 4).min(-1)                                  # [na, P]
                for L in range(4):
                    counts[i, mine, L] = (m > L).sum(-1)
                if want_ambiguous:
                    amb[i, mine] = ((np.abs(d2 - R2[None, None, :]) < AMBIGUOUS) & ~itself[:, None, :]).any(-1)
    return (counts, amb) if want_ambiguous else counts


def area_fp64(counts, radius, probe, n_points):
    """[N, 4] float64: sum over present slots of (4 pi / P) R_a^2 counts."""
    R = np.where(np.asarray(radius) > 0, np.asarray(radius, np.float64) + float(probe), 0.0)
    return (((4.0 * np.pi / n_points) * R * R)[:, :, None] * np.asarray(counts, np.float64)).sum(1)


def arrays(batch):
    """(xyz [N, 14, 3], radius [N, 14], chain [N]) float32 / int64 of a batch (B = 1, packed or padded: rows flattened), with the
    radii ``Context.sasa`` uses by default."""
    X = batch["X"].reshape(-1, 14, 3).cpu().numpy().astype(np.float32)
    rt = batch["residue_type"].reshape(-1).cpu().numpy()
    am = batch["atom_mask"].reshape(-1, 14).cpu().numpy()
    radius = np.asarray(rc.slot_radius, np.float32)[rt] * (am != 0)
    return X, radius.astype(np.float32), batch["chain_indices"].reshape(-1).cpu().numpy()


def seg_table(batch):
    host = batch.get("seg_offsets_host")
    if host is not None:
        return [int(x) for x in host]
    B, L = batch["residue_type"].shape
    return [s * L for s in range(B + 1)]


def make(n_res, seed, n_chains=2, zero_row=None):
    """B = 1 batch of ``synth.make_complex``; ``zero_row``: that row's atom_mask zeroed (a row without atoms)."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    b = protein_to_batch(synth.make_complex(n_res, seed, n_chains))
    if zero_row is not None:
        b["atom_mask"] = b["atom_mask"].clone()
        b["atom_mask"][0, zero_row] = 0
    return b


def ligand_near(batch, n_atoms, seed, spread=3.0):
    """[n_atoms, 4] float32 obstacle atoms scattered within ``spread`` A of a surface side-chain atom of the first chain."""
    X, radius, chain = arrays(batch)
    g = np.random.default_rng(seed)
    centre = X[radius > 0].mean(0)
    rows = np.nonzero((chain == chain[0]) & (radius[:, 5] > 0))[0]
    far = rows[np.argmax(np.linalg.norm(X[rows, 5] - centre, axis=1))]
    out = X[far, 5] + (X[far, 5] - centre) / np.linalg.norm(X[far, 5] - centre) * 3.0
    xyz = out + g.normal(size=(n_atoms, 3)) * spread / 2
    return np.concatenate([xyz, g.choice([1.7, 1.55, 1.52, 1.8], size=(n_atoms, 1))], 1).astype(np.float32)


# ---- tests -------------------------------------------------------------------------------------------------------------------------------
def test_pp_sasa_is_declared_bound_and_exported():
    import ctypes
    from packppi_amd.build import build_library
    from packppi_amd.lib import SYMBOLS
    body = re.sub(r"/\*.*?\*/", "", HEADER, flags=re.S)
    assert re.search(r"\bpp_status\s+pp_sasa\s*\(", body)
    assert "pp_sasa" in SYMBOLS
    assert 1 <= LIST_CAP <= 1024 and MAX_POINTS == 256
    assert hasattr(ctypes.CDLL(build_library(verbose=False)), "pp_sasa")


def test_sphere_points_are_unit_vectors_and_deterministic():
    from packppi_amd.analysis import sphere_points
    for P in (1, 2, 96, 250, 256):
        u = sphere_points(P)
        assert u.dtype == np.float32 and u.shape == (P, 3) and u.flags["C_CONTIGUOUS"]
        assert np.abs(np.linalg.norm(u.astype(np.float64), axis=1) - 1.0).max() <= 1e-7
        assert np.array_equal(u, sphere_points(P))
        k = np.arange(P, dtype=np.float64)
        z = 1.0 - (2.0 * k + 1.0) / P
        assert np.array_equal(u[:, 2], z.astype(np.float32))
    assert np.array_equal(sphere_points(1), np.float32([[1.0, 0.0, 0.0]]))
    u = sphere_points(96).astype(np.float64)
    assert np.abs(u.mean(0)).max() < 0.02                       # an even cover: the centroid sits at the origin
    with pytest.raises(ValueError):
        sphere_points(0)


def test_an_isolated_atom_is_exposed_on_every_level():
    from packppi_amd.analysis import sphere_points
    xyz = np.zeros((2, 14, 3), np.float32)
    xyz[1] = 100.0
    radius = np.zeros((2, 14), np.float32)
    radius[0, 1] = 1.7
    radius[1, 3] = 1.52
    for P in (1, 96):
        c = restate(xyz, radius, np.array([1, 2]), [0, 2], sphere_points(P), 1.4)
        assert (c[0, 1] == P).all() and (c[1, 3] == P).all() and c.sum() == 8 * P
    # a NaN coordinate: never buried, buries nothing
    xyz[1] = 0.5
    xyz[1, 3, 0] = np.nan
    c = restate(xyz, radius, np.array([1, 2]), [0, 2], sphere_points(96), 1.4)
    assert (c[0, 1] == 96).all() and (c[1, 3] == 96).all()


@pytest.mark.parametrize("n_res,seed", [(24, 5), (64, 11)])
def test_levels_nest_and_fp32_agrees_with_fp64_outside_ambiguous_points(n_res, seed):
    from packppi_amd.analysis import sphere_points
    b = make(n_res, seed)
    X, radius, chain = arrays(b)
    ob = ligand_near(b, 12, seed)
    pts = sphere_points(96)
    c32 = restate(X, radius, chain, [0, n_res], pts, 1.4, ob)
    c64, amb = restate(X, radius, chain, [0, n_res], pts, 1.4, ob, dtype=np.float64, want_ambiguous=True)
    assert (np.diff(c32, axis=-1) <= 0).all() and (np.diff(c64, axis=-1) <= 0).all()
    assert (c32[radius <= 0] == 0).all() and c32.max() <= 96
    frac = amb[radius > 0].mean()
    clear = ~amb.any(-1)
    print(f"make_complex({n_res}, {seed}): ambiguous points {frac:.2e}, atoms whose counts differ fp32/fp64 {(c32 != c64).any(-1).sum()}")
    assert frac <= 1e-3
    assert np.array_equal(c32[clear], c64[clear])
    # every level says something here: the chains touch, the ligand buries surface, and without it level 3 is level 2
    per_row = c32.sum(1)
    assert (per_row[:, 0] > per_row[:, 1]).any() and (per_row[:, 1] > per_row[:, 2]).any() and (per_row[:, 2] > per_row[:, 3]).any()
    bare = restate(X, radius, chain, [0, n_res], pts, 1.4)
    assert np.array_equal(bare[..., 3], bare[..., 2]) and np.array_equal(bare[..., :3], c32[..., :3])
    a = area_fp64(c32, radius, 1.4, 96)
    assert (a[:, 1] - a[:, 2] >= 0).all() and (a[:, 1] - a[:, 2]).sum() > 50.0


def test_the_new_selectors_parse_and_refuse():
    from packppi_amd.cli import eval_diffusion, proximal_optimize
    from packppi_amd.selection import device_selector
    assert device_selector("interface:sasa") == "interface" and device_selector("pocket", "hetero") == "pocket"
    assert device_selector("pocket", "hetero+water") == "pocket"
    assert device_selector("interface") is None and device_selector("A:4-9,B") is None and device_selector(None) is None
    with pytest.raises(ValueError, match="--obstacles"):
        device_selector("pocket")
    with pytest.raises(ValueError, match="--obstacles"):
        device_selector("pocket", "none")
    ev = ["--input", "x.pdb", "--outdir", "o", "--molprobity_clash_loc", "none", "--seed", "3"]
    a = eval_diffusion.parse_args(ev + ["--repack", "interface:sasa", "--sasa"])
    assert a.repack == "interface:sasa" and a.sasa
    assert eval_diffusion.parse_args(ev + ["--repack", "pocket", "--obstacles", "hetero"]).repack == "pocket"
    assert eval_diffusion.parse_args(ev).sasa is False
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(ev + ["--repack", "pocket"])
    with pytest.raises(SystemExit):
        eval_diffusion.parse_args(ev + ["--repack", "pocket", "--obstacles", "none"])
    po = ["--input", "x.pdb", "--outdir", "o", "--molprobity_clash_loc", "none"]
    assert proximal_optimize.parse_args(po + ["--repack", "pocket", "--obstacles", "hetero", "--sasa"]).sasa
    assert proximal_optimize.parse_args(po + ["--repack", "interface:sasa"]).repack == "interface:sasa"
    with pytest.raises(SystemExit):
        proximal_optimize.parse_args(po + ["--repack", "pocket"])
    from packppi_amd.cli import mutate
    m = mutate.build_parser().parse_args(["--input", "x.pdb", "--mutstr", "RA4A", "--outdir", "o", "--seed", "1", "--sasa"])
    assert m.sasa and not mutate.build_parser().parse_args(["--input", "x.pdb", "--mutstr", "RA4A", "--outdir", "o", "--seed", "1"]).sasa


def test_sasa_csv_format():
    from packppi_amd.analysis import SASA_CSV_HEADER, sasa_csv_text
    protein = dict(chain_id=np.array(["A", "A", "B"]), residue_index=np.array([7, 8, -2]), aaindex=np.array([0, 14, 5]))
    area = np.float32([[120.5, 80.25, 60.0, 59.5], [90.0, 0.0, 0.0, 0.0]])
    text = sasa_csv_text(protein, area, area[:, 1] - area[:, 2], area[:, 3] / area[:, 0])
    lines = text.split("\n")
    assert text.endswith("\n") and len(lines) == 5 and lines[-1] == ""
    assert lines[0] == SASA_CSV_HEADER == "chain,number,name,sasa_residue,sasa_chain,sasa_complex,sasa_ligand,bsa,exposure"
    assert lines[1] == f"A,7,{rc.resnames[0]},120.500,80.250,60.000,59.500,20.250,0.4938"
    assert lines[2] == f"A,8,{rc.resnames[14]},90.000,0.000,0.000,0.000,0.000,0.0000"
    assert lines[3] == f"B,-2,{rc.resnames[5]},0.000,0.000,0.000,0.000,0.000,0.0000"          # a row the ensemble dropped
