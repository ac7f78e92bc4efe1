"""A sampling run launches the layer-1 edge update of every evaluation on the context's LIVE rows only -- the rows with
``residue_mask != 0`` and at least one non-zero ``SC_D_mask`` entry; ``sample_partial`` also leaves out the call's fixed rows
(DESIGN.md section 4.8).  Nothing that launch computes for another row reaches the returned angles, so the results must not change
by one bit: every shape below is sampled twice, with ``PP_EDGE_LIVE=0`` (the launch over all rows) and with the default, in fresh
child processes (the switch is read once per process), and the angles, the trajectories and ``Context.saturated()`` are compared
with ``torch.equal``.

Libraries: the default one, ``libpackppi_hip.f32.so``, and ``libpackppi_hip.dbg.so`` with ``PP_EDGE_R=2`` -- the product
libraries run two-row workgroups only above three rows per CU, the diagnostics library can force them at these sizes (odd live
counts leave a pair workgroup with one row).  The T1124 fixture (739 rows) is the size at which the default library takes the mixed
launch with its work table.

Shapes: see ``_cases``.  The issue's ragged batch of 17, 40 and 33 residues cannot be PACKED (a packed context takes complexes
shorter than 32 residues only on their own: K = min(32, L) is one constant per context), so these lengths run as the padded batch
the library accepts for them -- its padding rows are masked rows on both sides of every boundary -- and a packed batch of 37, 40
and 33 residues runs next to it, both with dead rows on either side of each boundary.
"""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
N_SCHEDULE = 5                      # 4 reverse steps
ALA, GLY, LEU = 0, 7, 10


def _typed(n_res, seed, dead):
    """synth.make_complex(n_res, seed) with the residue types rewritten: rows in ``dead`` become GLY / ALA in turn, every other
    GLY / ALA becomes LEU; dead = None keeps the drawn types."""
    from packppi_amd import synth
    from packppi_amd.synth import rc
    p = synth.make_complex(n_res, seed)
    if dead is None:
        return p
    aatype = p["aaindex"].copy()
    assert rc.chi_angles_mask[ALA].sum() == 0 and rc.chi_angles_mask[GLY].sum() == 0 and rc.chi_angles_mask[LEU].sum() > 0
    no_chi = rc.chi_angles_mask[aatype].sum(-1) == 0
    aatype[no_chi] = LEU
    for k, i in enumerate(sorted(dead)):
        aatype[i] = GLY if k % 2 == 0 else ALA
    rng = np.random.default_rng(seed + 1000)
    chi = rng.uniform(-np.pi, np.pi, (n_res, 4)) * rc.chi_angles_mask[aatype]
    bb = np.nan_to_num(p["atom_positions"][:, :4]).astype(np.float64)
    xyz = synth.build_atom14(bb, aatype, chi)
    mask = rc.atom14_mask[aatype].astype(np.float64)
    xyz = np.where(mask[..., None] > 0, xyz, np.nan).astype(np.float32).astype(np.float64)
    return dict(p, atom_positions=xyz, atom_mask=mask, aaindex=aatype.astype(np.int64))


def _mask_residue(c, i):
    """Residue i of a one-complex batch masked out mid-chain, as featurize does for a missing backbone atom."""
    c.residue_mask[0, i] = 0.0
    for k in ("X", "atom_mask", "SC_D", "SC_D_mask", "BB_D", "BB_D_mask", "BB_D_sincos", "SC_D_sincos"):
        c[k][0, i] = 0
    for k in ("chi_1pi_periodic_mask", "chi_2pi_periodic_mask"):
        c[k][0, i] = False
    return c


ODD_DEAD = (1, 2, 7, 12, 13, 20, 26, 32)           # 33 - 8 = 25 live rows, first pair and last row included


def _cases():
    """name -> batch (CPU).  Built the same way in every child and in the list test."""
    from packppi_amd.batch import collate, pack
    from packppi_amd.featurize import protein_to_batch, protein_to_data
    from .conftest import load_golden
    out = {}
    out["odd_L33"] = protein_to_batch(_typed(33, 301, ODD_DEAD))                       # K = 32, odd live count
    out["L20_shortK"] = protein_to_batch(_typed(20, 302, (0, 5, 6, 19)))               # K = 20 < 32
    out["empty"] = protein_to_batch(_typed(24, 303, range(24)))                        # no live row at all
    out["identity"] = protein_to_batch(_typed(24, 304, ()))                            # no dead row
    out["masked_row"] = _mask_residue(protein_to_batch(_typed(40, 305, (3, 16, 18, 39))), 17)   # residue_mask == 0 mid-chain
    # dead rows on both sides of each boundary (rows 36 | 37 and 76 | 77 of the packed batch)
    out["packed_37_40_33"] = pack([protein_to_batch(_typed(37, 306, (0, 9, 36))), protein_to_batch(_typed(40, 307, (0, 21, 39))),
                                   protein_to_batch(_typed(33, 308, (0, 15)))])
    out["padded_17_40_33"] = collate([protein_to_data(_typed(17, 309, (0, 8, 16))), protein_to_data(_typed(40, 310, (0, 21, 39))),
                                      protein_to_data(_typed(33, 311, (0, 15, 32)))])
    out["T1124_mixed"] = load_golden("g4_T1124")[0]                                    # 739 rows: the mixed launch of the default library
    return out


def _expected_live(b):
    rm = b.residue_mask.reshape(-1).numpy()
    sc = b.SC_D_mask.reshape(-1, 4).numpy()
    return np.flatnonzero((rm != 0) & (sc != 0).any(-1)).astype(np.int32)


def _child_main(out_path):
    """Run in a fresh process (PACKPPI_LIB / PP_EDGE_LIVE / PP_EDGE_R in the environment): every shape, every entry point."""
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.weights import make_random_state_dict
    from .conftest import WEIGHT_SEED
    model = TDiffusionModule(make_random_state_dict(WEIGHT_SEED), device=DEV)
    sched = torch.linspace(1, 0, N_SCHEDULE)
    res = {}
    for name, b in _cases().items():
        ctx = model._context(b.to(DEV))
        g = torch.Generator().manual_seed(17)
        chi0 = (torch.rand(ctx.B, ctx.L, 4, generator=g) * 2 - 1) * 3.0 * b.SC_D_mask.reshape(ctx.B, ctx.L, 4)
        res[name + "/ode"] = ctx.sample(chi0, sched).cpu().numpy()
        res[name + "/ode_saturated"] = np.array(ctx.saturated())          # (the word is sticky: read after every entry point)
        res[name + "/seeded_sde"] = ctx.sample(chi0, sched, mode="sde", seed=5).cpu().numpy()
        res[name + "/seeded_sde_saturated"] = np.array(ctx.saturated())
        if name in ("odd_L33", "masked_row", "packed_37_40_33", "T1124_mixed"):
            n = ctx.n_rows
            g2 = torch.Generator().manual_seed(23)
            ref = (torch.rand(ctx.B, ctx.L, 4, generator=g2) * 2 - 1) * 3.0 * b.SC_D_mask.reshape(ctx.B, ctx.L, 4)
            for tag, fixed, fm, mode in (("every_second", (torch.arange(n) % 2 == 0), "renoise", "sde"),
                                         ("all", torch.ones(n, dtype=torch.bool), "hold", "ode")):
                chi, traj = ctx.sample_partial(chi0, ref, fixed, sched, mode, 9, fix_mode=fm, trajectory=True)
                res[f"{name}/partial_{tag}"] = chi.cpu().numpy()
                res[f"{name}/partial_{tag}_traj"] = traj.cpu().numpy()
                res[f"{name}/partial_{tag}_saturated"] = np.array(ctx.saturated())
        res[name + "/saturated"] = np.array(ctx.saturated())
    np.savez(out_path, **res)


def _lib_path(which):
    from packppi_amd import build
    return {"default": build.LIB, "f32": build.other_variant_path(), "dbg_R2": build.diag_variant_path()}[which]


@pytest.fixture(scope="module")
def runs():
    """{(library, PP_EDGE_LIVE): arrays} -- six child processes, started together, once for the module."""
    tmp = tempfile.mkdtemp(prefix="live_rows_")
    procs = {}
    for which in ("default", "f32", "dbg_R2"):
        lib = _lib_path(which)
        assert os.path.exists(lib), f"{lib} is missing (__graft_entry__.build() builds it)"
        for live in ("0", "1"):
            env = dict(os.environ, PACKPPI_LIB=lib, PP_EDGE_LIVE=live)
            if which == "dbg_R2":
                env["PP_EDGE_R"] = "2"
            out = os.path.join(tmp, f"{which}_{live}.npz")
            procs[(which, live)] = (subprocess.Popen(
                [sys.executable, "-c", f"import tests.test_live_rows as t; t._child_main({out!r})"],
                env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True), out)
    got = {}
    try:
        for key, (p, out) in procs.items():
            text, _ = p.communicate(timeout=600)
            assert p.returncode == 0, f"{key}: exit {p.returncode}\n{text[-3000:]}"
            got[key] = dict(np.load(out))
    finally:                        # a failure above must not leave a child on the GPU
        for p, _ in procs.values():
            if p.poll() is None:
                p.kill()
                p.wait()
        shutil.rmtree(tmp, ignore_errors=True)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["default", "f32", "dbg_R2"])
def test_live_launch_is_bit_identical(runs, which):
    """Every shape, every sampling entry point: PP_EDGE_LIVE=0 and the default give the same angles, trajectories and sticky word."""
    all_rows, live = runs[(which, "0")], runs[(which, "1")]
    assert sorted(all_rows) == sorted(live) and len(live) >= 8 * 3
    bad = []
    for k in sorted(live):
        a, b = torch.from_numpy(all_rows[k]), torch.from_numpy(live[k])
        if "saturated" not in k:
            assert torch.isfinite(b).all(), k
        if not torch.equal(a, b):
            bad.append((k, int((a != b).sum())))
    print(which, len(live), "arrays compared; differing:", bad)
    assert not bad


@pytest.mark.gpu
def test_the_runs_moved_the_live_rows(runs):
    """The comparison is not between two runs that did nothing: live rows moved, rows without an angle stayed at zero, and a run
    with every row fixed returned chi_ref's rows (the all-fixed launch has an empty list)."""
    r = runs[("default", "1")]
    b = _cases()["odd_L33"]
    live = _expected_live(b)
    assert len(live) == 33 - len(ODD_DEAD) and len(live) % 2 == 1
    chi = r["odd_L33/ode"].reshape(-1, 4)
    dead = np.setdiff1d(np.arange(33), live)
    assert np.all(chi[dead] == 0) and np.abs(chi[live]).max() > 0.1
    assert not np.array_equal(r["odd_L33/ode"], r["odd_L33/seeded_sde"])
    assert np.all(r["empty/ode"] == 0)
    g2 = torch.Generator().manual_seed(23)
    ref = ((torch.rand(1, 33, 4, generator=g2) * 2 - 1) * 3.0 * b.SC_D_mask.reshape(1, 33, 4)).numpy()
    assert np.array_equal(r["odd_L33/partial_all"], ref)
    assert np.array_equal(r["odd_L33/partial_every_second"].reshape(-1, 4)[0::2], ref.reshape(-1, 4)[0::2])


@pytest.mark.gpu
def test_live_row_list_matches_the_masks(weights):
    """The device scan against the numpy expression on the masks, on every shape and on 1500 rows (more rows than the scan's
    workgroup has threads)."""
    from packppi_amd.module import TDiffusionModule
    from .conftest import load_golden
    model = TDiffusionModule(weights, device=DEV)
    cases = dict(_cases(), S1500=load_golden("g5_S1500")[0])
    for name, b in cases.items():
        ctx = model._context(b.to(DEV))
        got = ctx.live_rows().cpu().numpy()
        want = _expected_live(b)
        print(name, "rows", ctx.n_rows, "live", len(want))
        assert got.dtype == np.int32 and np.array_equal(got, want), name
    assert len(_expected_live(cases["empty"])) == 0 and len(_expected_live(cases["identity"])) == 24


def test_dead_row_counts_of_the_fixtures():
    """The counts DESIGN.md section 4.8 quotes, from the committed fixtures (CPU)."""
    from .conftest import load_golden
    for name, rows, true_rows, live in (("g4_T1124", 739, 738, 569), ("g5_S1500", 1500, 1500, 1173)):
        b = load_golden(name)[0]
        assert b.residue_mask.numel() == rows and int(b.residue_mask.sum()) == true_rows
        assert len(_expected_live(b)) == live, (name, len(_expected_live(b)))
