"""Mutant modelling, host side: the mutant as a sampling input (featurize.mutant_model_data) and the NumPy
float32 restatement of pp_ctx_shell, which the GPU tests (tests/test_shell_gpu.py, tests/test_mutate_gpu.py) compare the kernel
with byte for byte.  The restatement itself is pinned here against the unmodified reference: the ``local_mask`` of the g11 goldens
(AffinityPrediction.get_local_subgraph, radius 10)."""
import os

import numpy as np
import pytest
import torch

from packppi_amd import constants as rc
from packppi_amd.featurize import (mutant_data, mutant_model_batch, mutant_model_data, parse_mutstr, protein_to_data,
                                   resolve_mutations)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
G11 = ("1BRS_LA87F", "1BRS_two_chains", "2FTL_ignored")
SHELL_ROWS = {"1BRS_LA87F": 28, "1BRS_two_chains": 38, "2FTL_ignored": 38}


# ---- the header comment of csrc/pp_shell.hip, restated in NumPy float32 -----------------------------------------------------------
def d2_f32(p, q):
    """((dx dx) + (dy dy)) + (dz dz) of broadcast float32 arrays [..., 3]: every operation rounded to fp32 on its own."""
    d = np.asarray(p, dtype=np.float32) - np.asarray(q, dtype=np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def near_numpy(xyz, offs, radius, mode="ca", atom_mask=None):
    """Per segment of the table ``offs`` the bool matrix near[n, j] = "row j is within the radius of row n" (CA mode: the CA pair;
    ATOM mode: some pair of present atoms), strict d2 < r2 in float32.  It depends on neither the seeds nor the chain flag."""
    xyz = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 14, 3)
    r2 = np.float32(radius) * np.float32(radius)
    out = []
    for a, b in zip(offs[:-1], offs[1:]):
        P = xyz[a:b]
        with np.errstate(invalid="ignore", over="ignore"):
            if mode == "ca":
                near = d2_f32(P[:, None, 1], P[None, :, 1]) < r2
            else:
                m = np.asarray(atom_mask).reshape(-1, 14)[a:b] != 0
                near = np.zeros((b - a, b - a), dtype=bool)
                for j in range(b - a):                      # one partner row at a time: [n, 14, 14] per step
                    pair = d2_f32(P[:, :, None, :], P[j][None, None, :, :]) < r2
                    near[:, j] = (pair & m[:, :, None] & m[j][None, None, :]).any(axis=(1, 2))
        out.append(near)
    return out


def shell_from_near(near, seeds, offs, chain=None):
    """(shell uint8 [N], count int32 [n_seg]): row n is in the shell iff a seed row j of its segment is near it (and, with ``chain``,
    lies in another chain).  j = n counts."""
    seeds = np.asarray(seeds).reshape(-1) != 0
    shell = np.zeros(offs[-1], dtype=np.uint8)
    count = np.zeros(len(offs) - 1, dtype=np.int32)
    for s, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        ok = near[s] & seeds[a:b][None, :]
        if chain is not None:
            c = np.asarray(chain).reshape(-1)[a:b]
            ok = ok & (c[:, None] != c[None, :])
        shell[a:b] = ok.any(axis=1)
        count[s] = int(shell[a:b].sum())
    return shell, count


def shell_numpy(xyz, seeds, offs, radius, mode="ca", atom_mask=None, chain=None):
    """(shell uint8 [N], count int32 [n_seg]) of pp_ctx_shell.  xyz [N, 14, 3]; seeds [N]; offs: the segment table (first rows, then
    N); chain [N] or None (= without PP_SHELL_OTHER_CHAIN).  Partners are rows of the same segment only."""
    return shell_from_near(near_numpy(xyz, offs, radius, mode, atom_mask), seeds, offs, chain)


def golden(case):
    return np.load(os.path.join(GOLD, f"g11_affinity_{case}.npz"))


def protein_1brs():
    z = np.load(os.path.join(GOLD, "g0_protein_1BRS.npz"))
    return {k[5:]: z[k] for k in z.files if k.startswith("prot.")}


def row_of(protein, chain, number):
    (rows,) = np.nonzero((np.asarray(protein["chain_id"]) == chain) & (np.asarray(protein["residue_index"]) == number))
    assert len(rows) == 1
    return int(rows[0])


def assert_rows_equal(a, b, rows):
    """Every tensor key of b (protein_to_data) is in a and equal on `rows`, torch.equal."""
    for k, v in b.items():
        if isinstance(v, torch.Tensor):
            assert torch.equal(a[k][rows], v[rows]), k
        else:
            assert a[k] == v, k


# ---- 1. the shell restatement against the reference's local masks ----------------------------------------------------------------
@pytest.mark.parametrize("case", G11)
def test_shell_restatement_reproduces_the_reference_local_mask(case):
    z = golden(case)
    L = z["ref.X"].shape[0]
    shell, count = shell_numpy(z["ref.X"], z["ref.mut_mask"], [0, L], 10.0)
    assert np.array_equal(shell, z["local_mask"][0].astype(np.uint8))
    assert count.tolist() == [SHELL_ROWS[case]] and int(z["ref.mut_mask"].sum()) == (2 if case == "1BRS_two_chains" else 1)
    # the fixtures are not borderline: no CA pair of a seed within 0.02 A of the radius
    ca = z["ref.X"][:, 1].astype(np.float64)
    d = np.sqrt(((ca[:, None] - ca[None, z["ref.mut_mask"] != 0]) ** 2).sum(-1))
    assert np.abs(d - 10.0).min() > 0.02


def test_shell_restatement_on_the_padded_batch_per_row():
    z = golden("padded_B2")
    B, L = z["ref.mut_mask"].shape
    shell, count = shell_numpy(z["ref.X"].reshape(B * L, 14, 3), z["ref.mut_mask"], [0, L, 2 * L], 10.0)
    assert np.array_equal(shell.reshape(B, L), z["local_mask"].astype(np.uint8))
    assert count.tolist() == [28, 38]


def test_shell_restatement_keeps_segments_apart_and_knows_both_modes():
    """Two copies of one three-residue toy in one table: seeds in the first copy reach nothing in the second; the atom mode sees a
    side-chain contact the CA mode does not; OTHER_CHAIN drops the seed's own chain."""
    xyz = np.zeros((3, 14, 3), np.float32)
    xyz[:, :, 0] = np.array([0.0, 6.0, 30.0], np.float32)[:, None]        # CAs at x = 0, 6, 30
    xyz[1, 5, 0] = 27.0                                                  # one side-chain atom of row 1 next to row 2
    am = np.zeros((3, 14), np.float32)
    am[:, :5] = 1
    am[1, 5] = 1
    two = np.concatenate([xyz, xyz])
    seeds = np.array([0, 0, 1, 0, 0, 0])
    assert shell_numpy(two, seeds, [0, 3, 6], 5.0)[0].tolist() == [0, 0, 1, 0, 0, 0]
    assert shell_numpy(two, seeds, [0, 3, 6], 5.0, "atom", np.concatenate([am, am]))[0].tolist() == [0, 1, 1, 0, 0, 0]
    assert shell_numpy(two, seeds, [0, 6], 5.0)[0].tolist() == [0, 0, 1, 0, 0, 1]              # one segment: the copy is reached
    chain = np.array([1, 2, 2, 1, 2, 2])
    sh, cnt = shell_numpy(two, seeds, [0, 3, 6], 5.0, "atom", np.concatenate([am, am]), chain)
    assert sh.tolist() == [0, 0, 0, 0, 0, 0] and cnt.tolist() == [0, 0]
    assert shell_numpy(two, np.array([0, 1, 0, 0, 0, 0]), [0, 3, 6], 7.0, "ca", None, chain)[0].tolist() == [1, 0, 0, 0, 0, 0]


# ---- 2. the mutant as a sampling input ---------------------------------------------------------------------------------------------
def test_la87f_row_is_a_phenylalanine_everything_else_is_the_wild_type():
    p = protein_1brs()
    wt = protein_to_data(p)
    mt = mutant_model_data(p, parse_mutstr("LA87F"), log=lambda s: None)
    r = row_of(p, "A", 87)
    assert rc.restypes[int(wt.residue_type[r])] == "L"
    assert rc.restypes[int(mt.residue_type[r])] == "F"
    assert int(mt.atom_mask[r].sum()) == 11 and mt.atom_mask[r].tolist() == [1.0] * 11 + [0.0] * 3
    assert mt.SC_D_mask[r].tolist() == [1, 1, 0, 0]
    assert not mt.SC_D[r].any() and not mt.SC_D_sincos[r].any()
    pi1 = torch.from_numpy(rc.chi_pi_periodic)[rc.restype_order["F"]].bool()
    assert torch.equal(mt.chi_1pi_periodic_mask[r], pi1 & mt.SC_D_mask[r].bool())
    assert torch.equal(mt.chi_2pi_periodic_mask[r], ~pi1 & mt.SC_D_mask[r].bool())
    assert mt.chi_1pi_periodic_mask[r].tolist() == [False, True, False, False]                  # PHE chi2 has period pi
    assert torch.equal(mt.X[r, :4], wt.X[r, :4]) and not mt.X[r, 4:].any() and wt.X[r, 4:].any()
    assert mt.mut_mask.dtype == torch.int64 and mt.mut_mask.sum() == 1 and mt.mut_mask[r] == 1
    assert mt.mutation_tag == "LA87F" and mt.num_nodes == wt.num_nodes
    others = torch.arange(wt.num_nodes) != r
    assert_rows_equal(mt, wt, others)
    # the wild-type dict is left untouched, and the mutant differs from what PackPPI-AP consumes where the issue says it does
    assert_rows_equal(protein_to_data(p), wt, torch.ones(wt.num_nodes, dtype=torch.bool))
    ap = mutant_data(p, parse_mutstr("LA87F"), log=lambda s: None)
    assert torch.equal(ap.residue_type_mut, mt.residue_type) and torch.equal(ap.atom_mask_mut, mt.atom_mask)
    b = mutant_model_batch(p, "LA87F", log=lambda s: None)
    assert b.num_proteins == 1 and b.max_size == wt.num_nodes and torch.equal(b.SC_D_mask[0], mt.SC_D_mask)


def test_mutations_to_alanine_and_glycine():
    p = protein_1brs()
    wt = protein_to_data(p)
    chain, number, aa = np.asarray(p["chain_id"]), np.asarray(p["residue_index"]), np.asarray(p["aaindex"])
    r_arg = int(np.nonzero(aa == rc.restype_order["R"])[0][0])
    r_trp = int(np.nonzero(aa == rc.restype_order["W"])[0][0])
    muts = [dict(wt="R", chain=str(chain[r_arg]), resseq=int(number[r_arg]), mt="A"),
            dict(wt="W", chain=str(chain[r_trp]), resseq=int(number[r_trp]), mt="G")]
    mt = mutant_model_data(p, muts, log=lambda s: None)
    assert not mt.SC_D_mask[r_arg].any() and int(mt.atom_mask[r_arg].sum()) == 5                # ALA: no chi, N CA C O CB
    assert not mt.SC_D_mask[r_trp].any() and int(mt.atom_mask[r_trp].sum()) == 4                # GLY: backbone only
    for r in (r_arg, r_trp):
        assert not mt.chi_1pi_periodic_mask[r].any() and not mt.chi_2pi_periodic_mask[r].any() and not mt.X[r, 4:].any()
    assert mt.mut_mask.sum() == 2 and mt.mutation_tag.count(",") == 1
    others = torch.ones(wt.num_nodes, dtype=torch.bool)
    others[[r_arg, r_trp]] = False
    assert_rows_equal(mt, wt, others)


def test_ignored_and_mismatched_mutations_behave_as_in_mutant_data():
    p = protein_1brs()
    wt = protein_to_data(p)
    every = torch.ones(wt.num_nodes, dtype=torch.bool)
    for bad in ("LZ87F", "LA87X"):                                       # no chain Z; X is none of the 20 types
        said, said_ap = [], []
        mt = mutant_model_data(p, parse_mutstr(bad), log=said.append)
        mutant_data(p, parse_mutstr(bad), log=said_ap.append)
        assert said == said_ap == [f"Ignore the mutation: {bad}"]
        assert mt.mut_mask.sum() == 0 and mt.mutation_tag == ""
        assert_rows_equal(mt, wt, every)
    for bad, what in (("GA87F", "inconsistent with wild-type L"), ("LA9999F", "matches 0 residues")):
        for fn in (mutant_model_data, mutant_data):
            with pytest.raises(ValueError, match=what):
                fn(p, parse_mutstr(bad), log=lambda s: None)
    # one lookup for both featurisers
    (hit,) = resolve_mutations(p, parse_mutstr("LA87F,LZ87F"), log=lambda s: None)
    assert int(hit[0].nonzero()) == row_of(p, "A", 87) and hit[1] == rc.restype_order["F"] and hit[2] == "LA87F"


def test_to_pdb_of_the_mutant_names_phe_at_a87():
    from packppi_amd.pdb_io import to_pdb
    p = protein_1brs()
    mt = mutant_model_data(p, parse_mutstr("LA87F"), log=lambda s: None)
    text = to_pdb(dict(p, atom_positions=mt.X.numpy(), atom_mask=mt.atom_mask.numpy(), aaindex=mt.residue_type.numpy()))
    lines = [ln for ln in text.splitlines() if ln.startswith("ATOM") and ln[21] == "A" and int(ln[22:26]) == 87]
    assert [ln[17:20] for ln in lines] == ["PHE"] * 11
    assert [ln[12:16].strip() for ln in lines] == ["N", "CA", "C", "O", "CB", "CG", "CD1", "CD2", "CE1", "CE2", "CZ"]
    wt_lines = [ln for ln in to_pdb(p).splitlines() if ln.startswith("ATOM") and ln[21] == "A" and int(ln[22:26]) == 87]
    assert [ln[17:20] for ln in wt_lines] == ["LEU"] * 8


# ---- 3. the surface ------------------------------------------------------------------------------------------------------------------
def test_cli_help_says_what_the_ddg_columns_are():
    from packppi_amd.cli import mutate
    text = " ".join(mutate.build_parser().format_help().split())
    assert "The AP model was trained with zeroed mutant angles, so it does not see the packed mutant." in text
    for flag in ("--input", "--mutstr", "--mutlist", "--ckpt_path", "--config_dir", "--seed", "--n_decoys", "--select", "--use_proximal",
                 "--radius", "--shell", "--fixed_mode", "--outdir", "--ap_ckpt", "--pre_ckpt_path"):
        assert flag in text, flag
    with pytest.raises(SystemExit):
        mutate.main(["--input", "x.pdb", "--outdir", "o", "--seed", "1"])                        # neither --mutstr nor --mutlist
