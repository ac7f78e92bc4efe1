"""Obstacle atoms, host side: the PDB reader, the batch plumbing, the command-line flag -- and the
restatement of the obstacle term that tests/test_obstacles_gpu.py measures the kernels against.

The restatement is oracle.ref_cpu's own clash loss (``atom14_coords``, ``between_residue_clash``, ``within_residue_violation``,
untouched) plus the term of DESIGN.md section 19 written in torch, differentiated by autograd and optimised as
``ref_cpu.proximal_optimizer`` optimises.  It is anchored here, on the CPU, to the UNMODIFIED oracle by the chain-as-obstacles
identity: remove chain B's rows from a two-chain complex, hand B's atoms in as obstacles, and chain A's per_res is what the
oracle gives on the full complex (B's slot 5 masked there and left out of the obstacle set: the reference excludes slot-5/slot-5
pairs, the obstacle term has no such rule)."""
import gzip
import os
import warnings

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import ref_cpu as O
from packppi_amd import constants as rc
from packppi_amd.batch import TENSOR_KEYS, Batch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIG = os.path.join(ROOT, "tests", "golden", "T1124_lig.pdb.gz")
VTF, TOL = 12.0, 0.5
ANCHOR_CASES = ((24, 5), (40, 7), (64, 11))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def cast(batch, dtype):
    """The batch with every floating tensor in ``dtype`` (the oracle computes in the dtype of batch.X)."""
    out = Batch()
    for k, v in batch.items():
        out[k] = v.to(dtype) if isinstance(v, torch.Tensor) and v.is_floating_point() else v
    return out


def obstacle_per_atom(xyz, radius, obst, tol):
    """[B, L, 14]: for own atom a in slots 4..13 with exists * radius = r_a != 0 the sum over obstacles o with r_o > 0 of
    max((r_a + r_o) - tol - sqrt(1e-10 + |p_a - q_o|^2), 0); zero in slots 0..3.  ``obst`` [M, 4] (x, y, z, radius)."""
    q = obst.to(xyz.dtype)
    d = torch.sqrt(1e-10 + ((xyz[..., None, :] - q[:, :3]) ** 2).sum(-1))                   # [B, L, 14, M]
    act = ((radius != 0)[..., None] & (q[:, 3] > 0)).to(xyz.dtype)
    err = act * F.relu((radius[..., None] + q[:, 3]) - tol - d)
    slot = (torch.arange(14) >= 4).to(xyz.dtype)
    return err.sum(-1) * slot


def residue_clash_obst(batch, chi, obst, vtf=VTF, tol=TOL, parts=False):
    """ref_cpu.residue_clash with the obstacle term added to the per-atom sums: [B, L]."""
    dt = batch["X"].dtype
    S, exists = batch["residue_type"], batch["atom_mask"]
    n_sc = exists[..., 4:].sum(-1)
    xyz = O.atom14_coords(batch["X"], S, batch["BB_D"], chi)
    radius = exists * torch.as_tensor(rc.between_radius, dtype=dt)[S]
    lo, up = rc.make_atom14_dists_bounds(overlap_tolerance=tol, bond_length_tolerance_factor=vtf)
    per_atom = (O.between_residue_clash(xyz, exists, radius, batch["residue_index"], tol)
                + O.within_residue_violation(xyz, exists, torch.as_tensor(lo, dtype=dt)[S], torch.as_tensor(up, dtype=dt)[S]))
    ob = obstacle_per_atom(xyz, radius, obst, tol)
    if parts:
        return ob[..., 4:].sum(-1) / (1e-10 + n_sc)
    return (per_atom + ob)[..., 4:].sum(-1) / (1e-10 + n_sc)


def clash_and_grad_obst(batch, chi, obst, vtf=VTF, tol=TOL):
    """(per_res, d mean(per_res) / d chi) by autograd, as ref_cpu.clash_and_grad."""
    x = chi.clone().requires_grad_(True)
    pr = residue_clash_obst(batch, x, obst, vtf, tol)
    pr.mean().backward()
    return pr.detach(), x.grad.detach()


def proximal_obst(batch, chi0, obst, vtf=VTF, tol=TOL, lamda=1.0, num_steps=50):
    """ref_cpu.proximal_optimizer (optimize.py:21-73) with residue_clash_obst in the mask and the loss:
    (per-step chi list, pre-step losses, mask [B, L])."""
    with torch.no_grad():
        pr = residue_clash_obst(batch, chi0, obst, vtf, tol)
        mask = (pr > pr.mean())[..., None].expand(-1, -1, 4)
    z = chi0 * mask
    x = z.clone().requires_grad_(True)
    opt = torch.optim.Adam([x], lr=1e-2)
    chis, losses = [], []
    for _ in range(num_steps):
        opt.zero_grad()
        xe = torch.where(mask, x * mask, chi0)
        loss = (torch.abs(xe - z) ** 2).sum(-1).mean() + lamda * residue_clash_obst(batch, xe, obst, vtf, tol).mean()
        loss.backward()
        opt.step()
        chis.append(torch.where(mask, x.detach().clone(), chi0))
        losses.append(loss.item())
    return chis, losses, mask[..., 0]


def chain_as_obstacles(L, seed):
    """(full batch with chain B's slot 5 masked, chain A's rows as a B = 1 batch, rows of A, seeded random chi [1, L, 4],
    fn(dtype) -> chain B's atoms at those angles as obstacles [M, 4] without its slot-5 atoms)."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    full = protein_to_batch(synth.make_complex(L, seed))
    rows_a = (full.chain_indices[0] == 1).nonzero().flatten()
    rows_b = (full.chain_indices[0] != 1).nonzero().flatten()
    full["atom_mask"] = full.atom_mask.clone()
    full["atom_mask"][0, rows_b, 5] = 0.0
    g = torch.Generator().manual_seed(1000 + seed)
    chi = ((torch.rand(1, L, 4, generator=g) * 2 - 1) * np.pi) * full.SC_D_mask
    part = Batch(num_proteins=1, max_size=int(rows_a.numel()))
    for k in TENSOR_KEYS:
        part[k] = full[k][:, rows_a]

    def obstacles(dtype):
        f = cast(full, dtype)
        xyz = O.atom14_coords(f["X"], f["residue_type"], f["BB_D"], chi.to(dtype))[0, rows_b]              # [Lb, 14, 3]
        rad = (f["atom_mask"] * torch.as_tensor(rc.between_radius, dtype=dtype)[f["residue_type"]])[0, rows_b]
        keep = rad > 0                                                          # slot 5 of B is masked: left out
        return torch.cat((xyz[keep], rad[keep][:, None]), 1)

    return full, part, rows_a, chi, obstacles


@pytest.mark.parametrize("L,seed", ANCHOR_CASES)
def test_restatement_reproduces_the_oracle_on_a_chain_as_obstacles(L, seed):
    """The anchor: restatement on chain A + chain B's atoms as obstacles == the unmodified oracle on the full complex, on A's rows,
    within 5e-6 in fp32 and 1e-12 in fp64 -- and the obstacle term is not idle in it."""
    full, part, rows_a, chi, obstacles = chain_as_obstacles(L, seed)
    for dtype, bound in ((torch.float32, 5e-6), (torch.float64, 1e-12)):
        want = O.residue_clash(cast(full, dtype), chi.to(dtype), VTF, TOL)[0, rows_a]
        got = residue_clash_obst(cast(part, dtype), chi[:, rows_a].to(dtype), obstacles(dtype), VTF, TOL)[0]
        d = (got - want).abs().max().item()
        print(f"L {L} seed {seed} {dtype}: max abs difference {d:.3g}")
        assert d <= bound, (dtype, d)
    share = residue_clash_obst(cast(part, torch.float64), chi[:, rows_a].double(), obstacles(torch.float64), VTF, TOL, parts=True)
    assert int((share > 0).sum()) >= 3, "the obstacle term must be active on several rows of chain A"


def test_restated_gradient_matches_finite_differences():
    """autograd of the restatement against a central difference of mean(per_res) in fp64, on an angle the obstacles push."""
    full, part, rows_a, chi, obstacles = chain_as_obstacles(24, 5)
    b, x, ob = cast(part, torch.float64), chi[:, rows_a].double(), obstacles(torch.float64)
    _, g = clash_and_grad_obst(b, x, ob)
    share = residue_clash_obst(b, x, ob, parts=True)[0]
    r = int(torch.argmax(share * (b.SC_D_mask[0, :, 0] > 0)))
    h = 1e-6
    xp, xm = x.clone(), x.clone()
    xp[0, r, 0] += h
    xm[0, r, 0] -= h
    fd = (residue_clash_obst(b, xp, ob).mean() - residue_clash_obst(b, xm, ob).mean()) / (2 * h)
    assert abs(fd.item() - g[0, r, 0].item()) <= 1e-6 * max(1.0, abs(fd.item())), (fd.item(), g[0, r, 0].item())


# ---- the reader ----------------------------------------------------------------------------------------------------------------------
def _rec(kind, serial, name, alt, resname, chain, resseq, x, y, z, occ, el):
    return f"{kind:<6}{serial:>5} {name:<4}{alt}{resname:>3} {chain}{resseq:>4}    {x:8.3f}{y:8.3f}{z:8.3f}{occ:6.2f}{0.0:6.2f}          {el:>2}"


HAND = "\n".join([
    _rec("ATOM", 1, " N  ", " ", "ALA", "A", 1, 0.0, 0.0, 0.0, 1.0, "N"),
    _rec("ATOM", 2, " CA ", " ", "ALA", "A", 1, 1.4, 0.0, 0.0, 1.0, "C"),
    _rec("ATOM", 3, " C  ", " ", "ALA", "A", 1, 2.0, 1.4, 0.0, 1.0, "C"),
    _rec("ATOM", 4, " O  ", " ", "ALA", "A", 1, 1.3, 2.4, 0.0, 1.0, "O"),
    _rec("ATOM", 5, " N  ", " ", "SEP", "A", 2, 3.3, 1.5, 0.0, 1.0, "N"),          # non-standard residue on ATOM records
    _rec("ATOM", 6, " P  ", " ", "SEP", "A", 2, 5.0, 3.0, 1.0, 1.0, "P"),
    _rec("ATOM", 7, " H  ", " ", "SEP", "A", 2, 3.6, 0.6, 0.0, 1.0, "H"),
    _rec("HETATM", 8, " C1 ", " ", "LIG", "A", 101, 10.0, 0.0, 0.0, 1.0, "C"),
    _rec("HETATM", 9, " O1 ", "A", "LIG", "A", 101, 11.0, 0.0, 0.0, 0.4, "O"),       # altloc pair: B has the higher occupancy
    _rec("HETATM", 10, " O1 ", "B", "LIG", "A", 101, 11.5, 0.5, 0.0, 0.6, "O"),
    _rec("HETATM", 11, " S1 ", " ", "LIG", "A", 101, 12.0, 0.0, 0.0, 1.0, "S"),
    _rec("HETATM", 12, "BR1 ", " ", "LIG", "A", 101, 13.0, 0.0, 0.0, 1.0, "BR"),
    _rec("HETATM", 13, "CL1 ", " ", "LIG", "A", 101, 14.0, 0.0, 0.0, 1.0, ""),        # blank element: two letters from column 13
    _rec("HETATM", 14, " F1 ", " ", "LIG", "A", 101, 15.0, 0.0, 0.0, 1.0, ""),        # blank element: one letter from column 14
    _rec("HETATM", 15, " H1 ", " ", "LIG", "A", 101, 10.5, 1.0, 0.0, 1.0, "H"),
    _rec("HETATM", 16, " D1 ", " ", "LIG", "A", 101, 10.5, -1.0, 0.0, 1.0, "D"),
    _rec("HETATM", 17, "1H2 ", " ", "LIG", "A", 101, 10.5, 0.0, 1.0, 1.0, ""),        # blank element, hydrogen by its name
    _rec("HETATM", 18, "ZN  ", " ", " ZN", "A", 201, 20.0, 0.0, 0.0, 1.0, "ZN"),
    _rec("HETATM", 19, " O  ", " ", "HOH", "A", 301, 30.0, 0.0, 0.0, 1.0, "O"),
    _rec("HETATM", 20, " I  ", " ", "IOD", "A", 401, 40.0, 0.0, 0.0, 1.0, "I"),
    _rec("HETATM", 21, "SE  ", " ", "SEY", "A", 402, 41.0, 0.0, 0.0, 1.0, "SE"),
    "END"]) + "\n"


@pytest.fixture()
def hand_pdb(tmp_path):
    p = tmp_path / "hand.pdb"
    p.write_text(HAND)
    return str(p)


def test_reader_on_a_hand_written_file(hand_pdb):
    from packppi_amd.pdb_io import obstacle_atoms
    msgs = []
    o = obstacle_atoms(hand_pdb, log=msgs.append)
    assert o["element"] == ["N", "P", "C", "O", "S", "BR", "CL", "F", "I", "SE"]
    assert o["resname"] == ["SEP", "SEP"] + ["LIG"] * 6 + ["IOD", "SEY"]
    assert o["chain"] == ["A"] * 10 and o["resseq"] == [2, 2] + [101] * 6 + [401, 402]
    assert o["xyz"].dtype == np.float32 and o["radius"].dtype == np.float32 and o["xyz"].shape == (10, 3)
    np.testing.assert_array_equal(o["radius"], np.float32([1.55, 1.80, 1.7, 1.52, 1.8, 1.85, 1.75, 1.47, 1.98, 1.90]))
    np.testing.assert_array_equal(o["xyz"][3], np.float32([11.5, 0.5, 0.0]))                  # the altloc with occupancy 0.6
    assert len(msgs) == 1 and "ZN" in msgs[0]
    with pytest.warns(UserWarning, match="ZN"):
        obstacle_atoms(hand_pdb)
    w = obstacle_atoms(hand_pdb, water=True, log=msgs.append)
    assert w["resname"].count("HOH") == 1 and len(w["element"]) == 11
    np.testing.assert_array_equal(w["xyz"][w["resname"].index("HOH")], np.float32([30.0, 0.0, 0.0]))
    # the lines for writing back: every record of the groups, as in the file (hydrogens and the ZN included), no water
    src = HAND.split("\n")
    assert o["lines"] == [ln for ln in src if ln[17:20] in ("SEP", "LIG", " ZN", "IOD", "SEY")]
    assert w["lines"] == [ln for ln in src if ln[17:20] in ("SEP", "LIG", " ZN", "IOD", "SEY", "HOH")]


def test_radius_tables():
    assert rc.van_der_waals_radius == {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8}
    assert rc.obstacle_radius == {"C": 1.7, "N": 1.55, "O": 1.52, "S": 1.8, "P": 1.80, "F": 1.47, "CL": 1.75, "BR": 1.85,
                                  "I": 1.98, "SE": 1.90}
    # the protein table is made of the same four numbers, and none is above the 1.8 the kernels' reach is built on
    assert set(np.unique(rc.between_radius)) <= {0.0, 1.7, 1.55, 1.52, 1.8}


def test_reader_on_T1124_with_its_ligands():
    from collections import Counter
    from packppi_amd.pdb_io import _atom_records, from_pdb_file, obstacle_atoms, parse_atom_records
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        o = obstacle_atoms(LIG)
    assert Counter(o["element"]) == {"C": 46, "O": 16, "N": 14, "S": 2} and o["xyz"].shape == (78, 3)
    assert Counter(o["resname"]) == {"SAH": 52, "TYR": 26}
    with gzip.open(LIG, "rt") as fh:
        het = [ln.rstrip("\n") for ln in fh if ln.startswith("HETATM")]
    assert len(het) == 132 and o["lines"] == het
    # the protein reader does not see any of it: the same dict as from the ATOM records alone
    p, q = from_pdb_file(LIG), parse_atom_records(_atom_records(LIG))
    assert sorted(p) == sorted(q) == ["aaindex", "atom_mask", "atom_positions", "b_factors", "chain_id", "residue_index"]
    for k in p:
        np.testing.assert_array_equal(p[k], q[k])
    assert len(p["aaindex"]) > 300 and "HETATM" not in "".join(_atom_records(LIG))


def test_lines_go_between_the_last_TER_and_END(hand_pdb):
    from packppi_amd import synth
    from packppi_amd.pdb_io import insert_obstacle_lines, obstacle_atoms, to_pdb
    text = to_pdb(synth.make_complex(12, 3))
    lines = obstacle_atoms(hand_pdb, log=lambda m: None)["lines"]
    out = insert_obstacle_lines(text, lines).split("\n")
    src = text.split("\n")
    at = max(i for i, ln in enumerate(src) if ln.startswith("TER")) + 1
    assert out[:at] == src[:at] and out[at:at + len(lines)] == lines and out[at + len(lines):] == src[at:]
    assert out[at + len(lines)].startswith("ENDMDL") and out[at + len(lines) + 1].startswith("END")
    assert insert_obstacle_lines(text, []) == text


# ---- batch plumbing ------------------------------------------------------------------------------------------------------------------
def _obst(M, seed):
    g = np.random.default_rng(seed)
    return dict(xyz=g.normal(size=(M, 3)).astype(np.float32) * 10, radius=g.choice([1.7, 1.55, 1.52, 1.8], M).astype(np.float32))


def _xyzr(o):
    return torch.from_numpy(np.concatenate([o["xyz"], o["radius"][:, None]], 1))


def test_a_batch_without_obstacles_has_exactly_todays_keys():
    from packppi_amd import synth
    from packppi_amd.batch import OBSTACLE_KEYS, pack, replicate, split
    from packppi_amd.featurize import protein_to_batch, protein_to_data
    p = synth.make_complex(40, 2)
    today = sorted(TENSOR_KEYS + ("num_proteins", "max_size", "num_nodes"))
    assert sorted(protein_to_batch(p)) == sorted(protein_to_batch(p, obstacles=None)) == today
    assert sorted(protein_to_data(p)) == sorted(TENSOR_KEYS + ("num_nodes",))
    pk = pack([protein_to_batch(p), protein_to_batch(synth.make_complex(36, 3))])
    assert sorted(pk) == sorted(TENSOR_KEYS + ("num_proteins", "max_size", "seg_offsets", "seg_offsets_host"))
    rp = replicate(protein_to_batch(p), 3)
    assert not any(k in rp for k in OBSTACLE_KEYS) and not any(k in split(protein_to_batch(p))[0] for k in OBSTACLE_KEYS)


def test_batch_functions_carry_the_obstacles():
    from packppi_amd import synth
    from packppi_amd.batch import pack, replicate, replicate_many, split
    from packppi_amd.featurize import mutant_data, mutant_model_data, protein_to_batch, protein_to_data
    pa, pb, pc = synth.make_complex(40, 2), synth.make_complex(36, 3), synth.make_complex(33, 4)
    oa, oc = _obst(7, 1), _obst(5, 2)
    a, b, c = protein_to_batch(pa, obstacles=oa), protein_to_batch(pb), protein_to_batch(pc, obstacles=oc)
    assert a.obstacle_xyzr.shape == (7, 4) and a.obstacle_xyzr.dtype == torch.float32 and a.X.shape == (1, 40, 14, 3)
    assert torch.equal(a.obstacle_xyzr, _xyzr(oa)) and a.obstacle_offsets.tolist() == [0, 7] == a.obstacle_offsets_host
    assert a.obstacle_offsets.dtype == torch.int32
    d = protein_to_data(pa, obstacles=oa)
    assert torch.equal(d.obstacle_xyzr, a.obstacle_xyzr) and d.X.shape == (40, 14, 3)
    # pack: blocks back to back, an empty range for the complex without
    pk = pack([a, b, c])
    assert torch.equal(pk.obstacle_xyzr, torch.cat([_xyzr(oa), _xyzr(oc)])) and pk.obstacle_offsets_host == [0, 7, 7, 12]
    assert pk.obstacle_offsets.tolist() == [0, 7, 7, 12] and pk.seg_offsets_host == [0, 40, 76, 109]
    assert pack([d, b]).obstacle_offsets_host == [0, 7, 7]
    # split of a B = 1 batch, clone, to
    s = split(a)[0]
    assert torch.equal(s.obstacle_xyzr, a.obstacle_xyzr) and s.obstacle_offsets_host == [0, 7]
    cl = a.clone()
    assert torch.equal(cl.obstacle_xyzr, a.obstacle_xyzr) and cl.obstacle_xyzr.data_ptr() != a.obstacle_xyzr.data_ptr()
    assert cl.obstacle_offsets_host == [0, 7]
    to = pk.to("cpu")
    assert torch.equal(to.obstacle_xyzr, pk.obstacle_xyzr) and to.obstacle_offsets.tolist() == [0, 7, 7, 12]
    # decoys share their group's range: one range per complex
    rm = replicate_many([a, b, c], 3)
    assert rm.obstacle_offsets_host == [0, 7, 7, 12] and rm.n_decoys == 3 and len(rm.seg_offsets_host) == 10
    assert torch.equal(rm.obstacle_xyzr, pk.obstacle_xyzr)
    r1 = replicate(a, 4)
    assert r1.obstacle_offsets_host == [0, 7] and torch.equal(r1.obstacle_xyzr, a.obstacle_xyzr)
    # the two mutant featurisers
    muts = [{"wt": rc.restypes[int(pa["aaindex"][4])], "chain": "A", "resseq": int(pa["residue_index"][4]), "mt": "A"}]
    for fn in (mutant_data, mutant_model_data):
        m = fn(pa, muts, log=lambda s: None, obstacles=oa)
        assert torch.equal(m.obstacle_xyzr, a.obstacle_xyzr) and m.obstacle_offsets_host == [0, 7]
        assert "obstacle_xyzr" not in fn(pa, muts, log=lambda s: None)


def test_bad_obstacles_are_refused():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    p = synth.make_complex(33, 4)
    for bad in (dict(xyz=np.float32([[0, 0, np.nan]]), radius=np.float32([1.7])),
                dict(xyz=np.float32([[0, 0, 0]]), radius=np.float32([-1.0])),
                dict(xyz=np.float32([[0, 0, 0]]), radius=np.float32([np.inf])),
                dict(xyz=np.float32([[0, 0, 0], [1, 1, 1]]), radius=np.float32([1.7]))):
        with pytest.raises(ValueError):
            protein_to_batch(p, obstacles=bad)


def test_collate_and_sample_sharded_refuse():
    from packppi_amd import synth
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_batch, protein_to_data
    from packppi_amd.parallel import sample_sharded
    pa, pb = synth.make_complex(40, 2), synth.make_complex(36, 3)
    with pytest.raises(ValueError, match="obstacle"):
        collate([protein_to_data(pa, obstacles=_obst(3, 1)), protein_to_data(pb)])
    assert collate([protein_to_data(pa), protein_to_data(pb)]).X.shape == (2, 40, 14, 3)
    with pytest.raises(ValueError, match="obstacle"):
        sample_sharded(None, [protein_to_batch(pa, obstacles=_obst(3, 1)), protein_to_batch(pb)], rank=0, world=1)
    with pytest.raises(ValueError, match="obstacle"):
        sample_sharded(None, {1: protein_to_batch(pa, obstacles=_obst(3, 1))}, lengths=[36, 40], rank=0, world=1)


def test_batch_key_watches_the_obstacle_tensor():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.lib import BatchKey
    a = protein_to_batch(synth.make_complex(33, 4), obstacles=_obst(5, 2))
    key = BatchKey(a)
    assert key.matches(a)
    a.obstacle_xyzr[0, 0] += 1.0
    assert not key.matches(a)


# ---- command lines -------------------------------------------------------------------------------------------------------------------
def test_command_lines_take_the_flag():
    from packppi_amd.cli import eval_diffusion, mutate, proximal_optimize
    base = {eval_diffusion: ["--input", "x.pdb", "--outdir", "o", "--molprobity_clash_loc", "m"],
            proximal_optimize: ["--input", "x.pdb", "--outdir", "o", "--molprobity_clash_loc", "m"],
            mutate: ["--input", "x.pdb", "--outdir", "o", "--mutstr", "RA47A", "--seed", "1"]}
    for mod, argv in base.items():
        assert mod.build_parser().parse_args(argv).obstacles == "none", mod.__name__
        for v in ("none", "hetero", "hetero+water"):
            assert mod.build_parser().parse_args(argv + ["--obstacles", v]).obstacles == v
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(argv + ["--obstacles", "ligand"])
        assert "network" in mod.build_parser().format_help().replace("\n", " ")


# ---- the placements the GPU tests use (made and checked here, on the CPU) --------------------------------------------------------------
def terminal_atoms(batch, chi):
    """(xyz fp64 [L, 14, 3], rows with at least one chi angle, their last present side-chain slot, that atom's radius)."""
    b = cast(batch, torch.float64)
    xyz = O.atom14_coords(b["X"], b["residue_type"], b["BB_D"], chi.double())[0]
    has = (batch.SC_D_mask[0].sum(-1) > 0) & (batch.residue_mask[0] > 0)
    rows = has.nonzero().flatten()
    last = torch.stack([(batch.atom_mask[0, r] > 0).nonzero().flatten().max() for r in rows])
    rad = torch.as_tensor(rc.between_radius)[batch.residue_type[0, rows], last]
    return xyz, rows, last, rad


def place_near_terminals(batch, chi, n_rows, per_row, lo, hi, seed, overlap=False):
    """[n_rows * per_row, 4] fp32 obstacle atoms around the terminal side-chain atoms of ``n_rows`` seeded rows.  ``overlap`` False:
    at a distance in [lo, hi] from the terminal atom; True: overlapping it by [lo, hi], i.e. at (r_a + r_o - TOL) - overlap."""
    xyz, rows, last, rad = terminal_atoms(batch, chi)
    g = np.random.default_rng(seed)
    pick = g.choice(len(rows), n_rows, replace=False)
    out = []
    for k in pick:
        p = xyz[rows[k], last[k]].numpy()
        for _ in range(per_row):
            u = g.normal(size=3)
            u /= np.linalg.norm(u)
            ro = float(g.choice([1.7, 1.55, 1.52, 1.8]))
            amount = g.uniform(lo, hi)
            dist = (float(rad[k]) + ro - TOL) - amount if overlap else amount
            out.append(np.r_[p + dist * u, ro])
    return torch.from_numpy(np.float32(out)), rows[pick]


def value_case():
    """Test 2: g2_ops_L33 at its seeded initial angles, 20 obstacle atoms 1.5-2.6 A from side-chain terminal atoms."""
    from .conftest import load_golden
    b, rest = load_golden("g2_ops_L33")
    chi = rest["init_chi_seed7"]
    ob, rows = place_near_terminals(b, chi, 10, 2, 1.5, 2.6, seed=33)
    return b, chi, ob, rows


def proximal_case():
    """Test 5: g3_proximal_L64 at its starting angles, 12 obstacle atoms overlapping the terminal atoms of three side chains by
    0.5-1.2 A."""
    from .conftest import load_golden
    b, rest = load_golden("g3_proximal_L64")
    chi = rest["init_chi_seed11"]
    ob, rows = place_near_terminals(b, chi, 3, 4, 0.5, 1.2, seed=PROX_SEED, overlap=True)
    return b, chi, ob, rows


PROX_SEED = 64


def test_value_case_is_not_marginal():
    """Every obstacle of test 2 overlaps its terminal atom by at least 0.1 A, and no atom-obstacle hinge sits within 1e-4 of zero (where
    fp32 and fp64 could disagree about the branch)."""
    b, chi, ob, rows = value_case()
    assert ob.shape == (20, 4)
    b64 = cast(b, torch.float64)
    xyz = O.atom14_coords(b64["X"], b64["residue_type"], b64["BB_D"], chi.double())
    radius = b64["atom_mask"] * torch.as_tensor(rc.between_radius, dtype=torch.float64)[b64["residue_type"]]
    d = torch.sqrt(1e-10 + ((xyz[..., None, :] - ob.double()[:, :3]) ** 2).sum(-1))
    hinge = ((radius[..., None] + ob.double()[:, 3]) - TOL - d)[0, :, 4:][(radius != 0)[0, :, 4:]]
    assert (hinge.abs() > 1e-4).all() and int((hinge > 0.1).sum()) >= 20
    share = residue_clash_obst(b64, chi.double(), ob.double(), parts=True)[0]
    assert (share[rows] > 0).all()


def test_proximal_case_is_well_conditioned():
    """Test 5's placement, checked with the restatement alone: the rows the obstacles overlap are in the clash mask; every first-step
    gradient entry of the mask is exactly zero or at least 1e-5 (below that Adam's first step, lr g / (|g| + eps), is decided by
    rounding); and the restatement's fp32 and fp64 runs have the same mask and, over the 10 steps the GPU test compares, losses
    within 5e-5 relative of each other -- the bounds of that test are met by the reference itself."""
    b, chi, ob, rows = proximal_case()
    assert ob.shape == (12, 4)
    c64, l64, m64 = proximal_obst(cast(b, torch.float64), chi.double(), ob.double(), num_steps=10)
    c32, l32, m32 = proximal_obst(b, chi, ob, num_steps=10)
    assert torch.equal(m32, m64) and m64[0, rows].all()
    _, g = clash_and_grad_obst(cast(b, torch.float64), chi.double(), ob.double())
    gm = g[0][m64[0]].abs()
    print("smallest non-zero first-step |g| in the mask:", float(gm[gm > 0].min()), "rows", rows.tolist())
    assert ((gm == 0) | (gm >= 1e-5)).all()
    assert np.allclose(l32, l64, rtol=5e-5, atol=0)
    share = residue_clash_obst(cast(b, torch.float64), chi.double(), ob.double(), parts=True)[0]
    assert (share[rows] > 0.1).all()
