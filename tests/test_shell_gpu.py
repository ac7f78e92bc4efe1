"""pp_ctx_shell on the device (csrc/pp_shell.hip) against its NumPy float32 restatement
(tests/test_mutate_host.py), byte for byte, and -- CA mode, radius 10 -- against the unmodified reference's ``local_mask`` goldens.

Shapes.  Goldens: L = 195 (one 256-row workgroup, one pass over the seed rows), L = 280 (two workgroups, two passes), their pack
(N = 670: workgroups that straddle segments) and the padded [2, 280] batch.  Synthetic two-chain complexes of 33, 64, 65 and 97
residues, alone and as the pack (97, 65, 97) -- N = 259, the last three rows in a workgroup of their own, the outer segments the
SAME complex, so they and the middle one overlap in space and a cross-segment leak shows."""
import ctypes as C

import numpy as np
import pytest
import torch

from .test_mutate_host import G11, SHELL_ROWS, golden, near_numpy, shell_from_near, shell_numpy

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LENS = (33, 64, 65, 97)
RADII = (4.0, 8.0, 10.0)


def _ctx(batch):
    from packppi_amd.functional import geometry_plan
    from packppi_amd.lib import Context
    return Context(geometry_plan(torch.device(DEV)), batch)


def case_data(case):
    from packppi_amd.featurize import mutant_data, parse_mutstr
    z = golden(case)
    p = {k[5:]: z[k] for k in z.files if k.startswith("prot.")}
    return mutant_data(p, parse_mutstr(str(z["mutstr"])), ddg=float(z["ddG"]), log=lambda s: None)


def _np(t):
    return t.detach().cpu().numpy()


# ---- 1. CA mode against the reference's local masks -----------------------------------------------------------------------------
@pytest.mark.parametrize("case", G11)
def test_ca_mode_on_a_golden_alone(case):
    from packppi_amd.batch import as_single
    z = golden(case)
    b = as_single(case_data(case)).to(DEV)
    shell, count = _ctx(b).shell(b.mut_mask, radius=10.0, mode="ca", want_count=True)
    assert shell.dtype == torch.bool and shell.shape == b.mut_mask.shape
    assert np.array_equal(_np(shell).astype(np.float32), z["local_mask"])
    L = b.max_size
    ref, cnt = shell_numpy(_np(b.X[0]), _np(b.mut_mask[0]), [0, L], 10.0)
    assert np.array_equal(_np(shell)[0].astype(np.uint8), ref)
    assert count.tolist() == cnt.tolist() == [SHELL_ROWS[case]]


def test_ca_mode_on_the_goldens_packed_and_padded():
    from packppi_amd.batch import collate_affinity, pack
    datas = {c: case_data(c) for c in G11}
    pb = pack([datas[c] for c in G11], trim=False).to(DEV)
    assert pb.seg_offsets_host == [0, 195, 390, 670]
    shell, count = _ctx(pb).shell(pb.mut_mask, want_count=True)
    want = np.concatenate([golden(c)["local_mask"][0] for c in G11])
    assert np.array_equal(_np(shell)[0].astype(np.float32), want)
    assert count.tolist() == [SHELL_ROWS[c] for c in G11]
    ref, _ = shell_numpy(_np(pb.X[0]), _np(pb.mut_mask[0]), pb.seg_offsets_host, 10.0)
    assert np.array_equal(_np(shell)[0].astype(np.uint8), ref)
    # the padded [2, 280] batch: its rows are the segments, padding rows included
    z = golden("padded_B2")
    padded = collate_affinity([datas[str(c)] for c in z["cases"]]).to(DEV)
    shell, count = _ctx(padded).shell(padded.mut_mask, want_count=True)
    assert shell.shape == (2, 280) and np.array_equal(_np(shell).astype(np.float32), z["local_mask"])
    assert count.tolist() == [28, 38]


# ---- 2. both modes on synthetic complexes -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def complexes():
    """The four synthetic complexes on the device; in each, one row that has atoms loses its whole atom_mask."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    out = {}
    for n in LENS:
        b = protein_to_batch(synth.make_complex(n, 170 + n))
        am = b.atom_mask.clone()
        am[0, n // 3] = 0.0
        b["atom_mask"] = am
        out[n] = b.to(DEV)
    gly = sum(int((b.atom_mask[0].sum(-1) == 4).sum()) for b in out.values())
    assert gly >= 2, "the synthetic complexes hold no glycine rows"
    return out


def _moved(xyz, amask):
    """xyz with the side-chain atoms of one residue put 30 A from its CA, towards the row whose CA is closest to 30 A away:
    (xyz', row, target row).  A pre-filter that trusts per-type side-chain extents would never look at such a pair."""
    ca = xyz[:, 1].astype(np.float64)
    d = np.sqrt(((ca[:, None] - ca[None]) ** 2).sum(-1))
    d[(amask != 0).sum(-1) < 7, :] = 1e9            # the moved row has a side chain worth the name
    d[:, amask[:, 1] == 0] = 1e9                    # the target row has its CA
    r, f = np.unravel_index(np.argmin(np.abs(d - 30.0)), d.shape)
    out = xyz.copy()
    out[r, 4:] = (ca[r] + 30.0 * (ca[f] - ca[r]) / d[r, f]).astype(np.float32)
    return out, int(r), int(f)


def _moved_matters(xyz, moved, amask, r, f, offs):
    """With row r the only seed, in atom mode, some radius puts the target row in the shell only because of the moved atoms."""
    seeds = np.zeros(len(xyz), np.uint8)
    seeds[r] = 1
    return any(shell_numpy(moved, seeds, offs, rad, "atom", amask)[0][f] == 1 and shell_numpy(xyz, seeds, offs, rad, "atom", amask)[0][f] == 0
               for rad in RADII)


def _seed_sets(a, b, n):
    """none, one row, the first and last row of the segment [a, b), all its rows -- over the n rows of the batch."""
    sets = {}
    for name, rows in (("none", []), ("one", [a + (b - a) // 2]), ("ends", [a, b - 1]), ("all", list(range(a, b)))):
        s = np.zeros(n, np.uint8)
        s[rows] = 1
        sets[name] = s
    return sets


def _run_matrix(batch, offs, seed_sets, extra_xyz=()):
    """Every (xyz, mode, radius, seeds, chain flag) on one context against the restatement; returns the number of launches."""
    ctx = _ctx(batch)
    n = offs[-1]
    amask, chain = _np(batch.atom_mask[0]), _np(batch.chain_indices[0])
    gen = torch.Generator().manual_seed(n)
    chi = ((torch.rand(1, n, 4, generator=gen) * 2 - 1) * np.pi).to(DEV) * batch.SC_D_mask
    built = ctx.atom14(chi)
    variants = [("batch X", None, _np(batch.X[0])), ("atom14", built, _np(built[0]))]
    for name, arr in extra_xyz:
        variants.append((name, torch.from_numpy(arr).to(DEV).reshape(1, n, 14, 3), arr))
    launches, hits = 0, 0
    for vname, dev_xyz, host_xyz in variants:
        for mode in ("ca", "atom"):
            for radius in RADII:
                near = near_numpy(host_xyz, offs, radius, mode, amask)
                for sname, seeds in seed_sets.items():
                    for other in (False, True):
                        want, want_cnt = shell_from_near(near, seeds, offs, chain if other else None)
                        got, cnt = ctx.shell(torch.from_numpy(seeds).reshape(1, n), radius=radius, mode=mode, other_chain=other,
                                             xyz=dev_xyz, want_count=True)
                        got = _np(got)[0].astype(np.uint8)
                        where = (vname, mode, radius, sname, other)
                        assert np.array_equal(got, want), (where, np.nonzero(got != want)[0][:8])
                        assert cnt.tolist() == want_cnt.tolist() == [int(got[a:b].sum()) for a, b in zip(offs[:-1], offs[1:])], where
                        launches += 1
                        hits += int(want.sum())
    assert hits > 0
    return launches


@pytest.mark.parametrize("n", LENS)
def test_both_modes_on_a_complex_alone(n, complexes):
    b = complexes[n]
    amask, X = _np(b.atom_mask[0]), _np(b.X[0])
    moved, r, f = _moved(X, amask)
    assert _moved_matters(X, moved, amask, r, f, [0, n])
    seeds = np.zeros(n, np.uint8)
    seeds[r] = 1
    sets = _seed_sets(0, n, n)
    sets["moved row"] = seeds
    assert _run_matrix(b, [0, n], sets, extra_xyz=[("moved 30 A", moved)]) == 3 * 2 * 3 * 5 * 2
    # a row without a present atom is in no atom shell and seeds none, but its CA still counts in CA mode
    ctx, z = _ctx(b), n // 3
    every = torch.ones(1, n, dtype=torch.uint8)
    assert not bool(ctx.shell(every, radius=10.0, mode="atom")[0, z]) and bool(ctx.shell(every, radius=10.0, mode="ca")[0, z])
    only = torch.zeros(1, n, dtype=torch.uint8)
    only[0, z] = 1
    assert int(ctx.shell(only, radius=10.0, mode="atom").sum()) == 0 and bool(ctx.shell(only, radius=4.0, mode="ca")[0, z])


def test_both_modes_packed_seeds_in_the_middle_segment(complexes):
    from packppi_amd.batch import pack
    pb = pack([complexes[97], complexes[65], complexes[97]])
    offs = pb.seg_offsets_host
    assert offs == [0, 97, 162, 259]
    sets = _seed_sets(97, 162, 259)
    sets["every row"] = np.ones(259, np.uint8)
    amask = _np(pb.atom_mask[0])
    moved_mid, r, f = _moved(_np(pb.X[0, 97:162]), amask[97:162])
    moved = _np(pb.X[0]).copy()
    moved[97:162] = moved_mid
    assert _moved_matters(_np(pb.X[0]), moved, amask, 97 + r, 97 + f, offs)
    sets["moved row"] = np.zeros(259, np.uint8)
    sets["moved row"][97 + r] = 1
    _run_matrix(pb, offs, sets, extra_xyz=[("moved 30 A", moved)])
    # seeds in the middle segment only: nothing outside it is ever in the shell, although the outer complexes overlap it in space
    ctx = _ctx(pb)
    for mode in ("ca", "atom"):
        sh, cnt = ctx.shell(torch.from_numpy(sets["all"]).reshape(1, -1), radius=10.0, mode=mode, want_count=True)
        assert not sh[0, :97].any() and not sh[0, 162:].any() and sh[0, 97:162].any()
        assert cnt.tolist() == [0, int(sh.sum()), 0]
    ca = _np(pb.X[0, :, 1])
    assert np.sqrt(((ca[97:162, None] - ca[None, :97]) ** 2).sum(-1)).min() < 4.0            # they do overlap


# ---- 3. refusals ------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments(complexes):
    from packppi_amd import lib as L
    from packppi_amd.batch import Batch
    lib = L.load()
    b = complexes[33]
    ctx = _ctx(b)
    seeds = torch.ones(33, dtype=torch.uint8, device=DEV)
    out = torch.zeros(33, dtype=torch.uint8, device=DEV)
    st = L._stream(torch.device(DEV))
    null = C.c_void_p(0)

    def call(handle=None, s=seeds, mode=0, radius=10.0, flags=0, o=out):
        status = lib.pp_ctx_shell(ctx.handle if handle is None else handle, L._ptr(s) if s is not None else null, mode, radius, flags,
                                  null, L._ptr(o) if o is not None else null, null, st)
        return status, lib.pp_last_error()

    assert call()[0] == 0
    cases = [dict(handle=null), dict(s=None), dict(o=None), dict(mode=2), dict(mode=-1), dict(flags=2), dict(flags=3),
             dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(radius=float("inf"))]
    for kw in cases:
        status, msg = call(**kw)
        assert status == 1 and b"pp_ctx_shell" in msg, kw
    bare = Batch(X=b.X, residue_type=b.residue_type, BB_D=b.BB_D, num_proteins=1, max_size=33)
    bare_ctx = _ctx(bare)
    assert lib.pp_ctx_shell(bare_ctx.handle, L._ptr(seeds), 1, 10.0, 0, null, L._ptr(out), null, st) == 1          # no atom_mask
    assert lib.pp_ctx_shell(bare_ctx.handle, L._ptr(seeds), 0, 10.0, 1, null, L._ptr(out), null, st) == 1          # no chain_indices
    assert lib.pp_ctx_shell(bare_ctx.handle, L._ptr(seeds), 0, 10.0, 0, null, L._ptr(out), null, st) == 0
    torch.cuda.synchronize()
    assert bool(out.all())                                                                         # every CA is its own seed
    with pytest.raises(ValueError, match="mode"):
        ctx.shell(seeds, mode="cb")
    with pytest.raises(ValueError, match="seeds has"):
        ctx.shell(seeds[:-1])
    with pytest.raises(ValueError, match="xyz has"):
        ctx.shell(seeds, xyz=b.X[:, :-1])
    with pytest.raises(RuntimeError, match="radius"):
        ctx.shell(seeds, radius=0.0)
