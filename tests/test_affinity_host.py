"""PackPPI-AP on the host: featurisation, local mask and weight contract against the reference's own outputs
(tests/golden/g11_affinity_*.npz, tools/oracle/make_golden_affinity.py), and the new C ABI symbols."""
import os
import re

import numpy as np
import pytest
import torch

from packppi_amd import weights as W
from packppi_amd.affinity import AffinityPrediction, mutant_view
from packppi_amd.batch import AFFINITY_KEYS, Batch, as_single, collate_affinity, pack
from packppi_amd.featurize import mutant_data, parse_mutstr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
CASES = ("1BRS_LA87F", "1BRS_two_chains", "2FTL_ignored")
NEW = ("pp_affinity_create", "pp_affinity_destroy", "pp_affinity_encode", "pp_affinity_predict")


def golden(case):
    return np.load(os.path.join(GOLD, f"g11_affinity_{case}.npz"))


def protein(z):
    return {k[5:]: z[k] for k in z.files if k.startswith("prot.")}


def case_data(case):
    z = golden(case)
    return mutant_data(protein(z), parse_mutstr(str(z["mutstr"])), ddg=float(z["ddG"]), log=lambda s: None)


@pytest.mark.parametrize("case", CASES)
def test_mutant_data_equals_reference(case):
    z = golden(case)
    d = case_data(case)
    for k in AFFINITY_KEYS + ("ddg",):
        ref = torch.from_numpy(z["ref." + k])
        assert d[k].dtype == ref.dtype, k
        assert torch.equal(d[k], ref), k


def test_trap1_mutated_row_has_mask_but_zero_sincos():
    d = case_data("1BRS_LA87F")
    i = int(d["mut_mask"].argmax())
    assert int(d["mut_mask"].sum()) == 1
    assert d["SC_D_mask_mut"][i, :2].tolist() == [1.0, 1.0]          # L -> F: chi1, chi2 atoms exist in the wild type
    assert not d["SC_D_sincos_mut"][i].any() and not d["SC_D_mut"][i].any()


def test_collate_equals_reference():
    z = golden("padded_B2")
    b = collate_affinity([case_data(c) for c in [str(x) for x in z["cases"]]])
    for k in AFFINITY_KEYS + ("ddg",):
        assert torch.equal(b[k], torch.from_numpy(z["ref." + k])), k


def test_parse_mutstr():
    assert parse_mutstr("RA47A,EA48A") == [{"wt": "R", "mt": "A", "chain": "A", "resseq": 47},
                                           {"wt": "E", "mt": "A", "chain": "A", "resseq": 48}]
    assert parse_mutstr("KI115W")[0]["resseq"] == 115


def test_wild_type_mismatch_raises():
    p = protein(golden("1BRS_LA87F"))
    with pytest.raises(ValueError, match="inconsistent with wild-type L"):
        mutant_data(p, parse_mutstr("AA87F"))


def test_ignored_mutations_leave_wild_type():
    p = protein(golden("1BRS_LA87F"))
    msgs = []
    d = mutant_data(p, parse_mutstr("LZ87F,LA87X"), log=msgs.append)
    assert msgs == ["Ignore the mutation: LZ87F", "Ignore the mutation: LA87X"]
    assert not d["mut_mask"].any()
    assert torch.equal(d["residue_type_mut"], d["residue_type"])
    assert torch.equal(d["SC_D_sincos_mut"], d["SC_D_sincos"])
    X = as_single(d)["X"]
    assert not AffinityPrediction.get_local_subgraph(X[:, :, 1, :], as_single(d)["mut_mask"]).any()


def test_mutation_matches_raw_residue_number():
    # chain D of 1BRS is numbered from 1 again: D39 is found by its PDB number, not by the chain-offset residue_index
    d = case_data("1BRS_two_chains")
    p = protein(golden("1BRS_two_chains"))
    rows = np.where(d["mut_mask"].numpy() == 1)[0]
    assert [(str(p["chain_id"][r]), int(p["residue_index"][r])) for r in rows] == [("A", 89), ("D", 39)]


@pytest.mark.parametrize("case", CASES)
def test_local_subgraph_equals_reference(case):
    z = golden(case)
    b = as_single(case_data(case))
    local = AffinityPrediction.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"])
    assert torch.equal(local, torch.from_numpy(z["local_mask"]))


def test_local_subgraph_padded_and_t1124():
    z = golden("padded_B2")
    b = collate_affinity([case_data(c) for c in [str(x) for x in z["cases"]]])
    assert torch.equal(AffinityPrediction.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"]), torch.from_numpy(z["local_mask"]))
    import gzip
    import tempfile
    from packppi_amd.pdb_io import from_pdb_file
    zt = golden("T1124")
    with gzip.open(os.path.join(GOLD, "T1124_lig.pdb.gz"), "rt") as fh, tempfile.NamedTemporaryFile("w", suffix=".pdb") as out:
        out.write(fh.read())
        out.flush()
        p = from_pdb_file(out.name)
    b = as_single(mutant_data(p, parse_mutstr(str(zt["mutstr"]))))
    assert torch.equal(AffinityPrediction.get_local_subgraph(b["X"][:, :, 1, :], b["mut_mask"]), torch.from_numpy(zt["local_mask"]))


@pytest.mark.parametrize("mode", ["network", "linear"])
def test_weight_keys_equal_reference_state_dict(mode):
    z = golden("1BRS_LA87F")
    assert [n for n, _ in W.affinity_weight_spec(mode)] == [str(k) for k in z[f"keys.{mode}"]]


def test_weight_counts_match_header():
    hdr = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    n_net = int(re.search(r"#define PP_AFF_N_WEIGHTS (\d+)u", hdr).group(1))
    n_lin = int(re.search(r"#define PP_AFF_N_WEIGHTS_LINEAR (\d+)u", hdr).group(1))
    count = lambda mode: sum(int(np.prod(s)) for _, s in W.affinity_head_spec(mode))
    assert (count("network"), count("linear")) == (n_net, n_lin)


def test_missing_key_is_named():
    sd = W.make_random_affinity_state_dict(3)
    del sd["mutation_fusion.2.bias"]
    with pytest.raises(RuntimeError, match="mutation_fusion.2.bias"):
        W.check_affinity_state_dict(sd)
    assert "mutation_fusion.2.bias" not in W.check_affinity_state_dict(W.make_random_affinity_state_dict(3, "linear"), "linear")


def test_esm_mode_refused():
    with pytest.raises(NotImplementedError, match="esm"):
        AffinityPrediction({}, {}, mode="esm", device="cuda")
    with pytest.raises(ValueError, match="Invalid mode"):
        AffinityPrediction({}, {}, mode="bogus", device="cuda")


def test_mutation_branch_weights_layout():
    sd = W.make_random_affinity_state_dict(5)
    m = W.mutation_branch_state_dict(sd)
    assert [(k, tuple(v.shape)) for k, v in m.items()] == [(n, tuple(s)) for n, s in W.weight_spec()]
    emb = m["encoder.node_embedding.weight"]
    assert torch.equal(emb[:, :35], sd["mutation_encoder.node_embedding.weight"]) and not emb[:, 35:].any()
    assert all(not v.any() for k, v in m.items() if k.startswith("decoder_score."))
    assert torch.equal(m["mpnn.mpnn_layers.2.edge_dense.W_out.bias"], sd["mutation_mpnn.mpnn_layers.2.edge_dense.W_out.bias"])


def test_pack_keeps_mutation_keys_and_rows():
    ds = [case_data(c) for c in CASES]
    p = pack(ds, trim=False)
    assert p["seg_offsets_host"] == [0, 195, 390, 670]
    assert torch.equal(p["ddg"], torch.stack([d["ddg"] for d in ds]))
    assert torch.equal(p["residue_type_mut"][0, 195:390], ds[1]["residue_type_mut"])
    mt = mutant_view(p)
    assert mt["SC_D_sincos"] is p["SC_D_sincos_mut"] and mt["residue_mask"] is p["residue_mask"]


def test_abi_declared_bound_exported():
    hdr = open(os.path.join(ROOT, "include", "packppi_hip.h")).read()
    from packppi_amd import lib as L
    for s in NEW:
        assert re.search(r"\b%s\(" % s, hdr), s
        assert s in L.SYMBOLS, s
    so = os.path.join(ROOT, "packppi_amd", "csrc", "libpackppi_hip.so")
    if os.path.exists(so):
        import ctypes
        h = ctypes.CDLL(so)
        for s in NEW:
            assert hasattr(h, s), s
