"""Pins oracle/ref_affinity.py, the CPU oracle of PackPPI-AP, to the tensors the unmodified reference wrote into
tests/golden/g11_affinity_*.npz (tools/oracle/make_golden_affinity.py), before anything on the GPU relies on it.  No GPU.

Bounds are those tests/test_affinity_gpu.py holds the HIP path to: 1e-4 on the h tensors, 1e-4 + 1e-4 |ref| on ddg, 1e-4
relative on the loss; the fp32 oracle must meet them.  Every test also prints how far the fp32 oracle is from the fp64 oracle:
the conditioning figure tests/test_affinity_kernels.py scales its bounds with.
"""
import gzip
import os

import numpy as np
import pytest
import torch

from oracle import ref_affinity as A
from packppi_amd.batch import as_single, collate_affinity
from packppi_amd.featurize import mutant_data, parse_mutstr
from packppi_amd.weights import make_random_affinity_state_dict, make_random_state_dict

from .conftest import GOLD, WEIGHT_SEED

AFF_SEED = 20261016
CASES = ("1BRS_LA87F", "1BRS_two_chains", "2FTL_ignored")


def golden(case):
    return np.load(os.path.join(GOLD, f"g11_affinity_{case}.npz"))


def case_data(case):
    z = golden(case)
    p = {k[5:]: z[k] for k in z.files if k.startswith("prot.")}
    return mutant_data(p, parse_mutstr(str(z["mutstr"])), ddg=float(z["ddG"]), log=lambda s: None)


def batch_of(case):
    if case == "padded_B2":
        return collate_affinity([case_data(str(c)) for c in golden(case)["cases"]])
    return as_single(case_data(case))


def dist(a, ref):
    return float((a.double().reshape(-1) - torch.as_tensor(ref).double().reshape(-1)).abs().max())


@pytest.fixture(scope="module")
def pret_sd():
    return make_random_state_dict(WEIGHT_SEED)


@pytest.fixture(scope="module", autouse=True)
def _threads():
    n = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    torch.set_num_threads(n)


@pytest.mark.parametrize("case", CASES + ("padded_B2",))
def test_oracle_against_reference_tensors(case, pret_sd):
    z = golden(case)
    b = batch_of(case)
    b64, pret64 = A.to_double(b), A.to_double(pret_sd)
    ap = make_random_affinity_state_dict(AFF_SEED, "network")
    lin = make_random_affinity_state_dict(AFF_SEED, "linear")
    ap64, lin64 = A.to_double(ap), A.to_double(lin)
    with torch.no_grad():
        local = A.local_subgraph(b["X"][:, :, 1, :], b["mut_mask"])
        assert torch.equal(local, torch.from_numpy(z["local_mask"]).reshape(local.shape))
        assert torch.equal(A.local_subgraph(b64["X"][:, :, 1, :], b64["mut_mask"]), local)     # the arbiter's subgraph is the same
        out, out64 = {}, {}
        for o, a_sd, l_sd, p_sd, bb in ((out, ap, lin, pret_sd, b), (out64, ap64, lin64, pret64, b64)):
            mt = A.mutant_view(bb)
            o["h_pret_wt"], o["h_pret_mt"] = A.pret_feature(p_sd, bb), A.pret_feature(p_sd, mt)
            o["h_wt"] = A.encode(a_sd, bb, o["h_pret_wt"], local)
            o["h_mt"] = A.encode(a_sd, mt, o["h_pret_mt"], local)
            for mode in ("network", "linear"):
                o[f"{mode}.loss"], o[f"{mode}.ddg"], o[f"{mode}.ddg_inv"] = A.forward(a_sd if mode == "network" else l_sd, p_sd, bb, mode)
    for k in sorted(out):
        print(f"{case} {k}: fp32 oracle vs reference {dist(out[k], z[k]):.3e}, fp32 oracle vs fp64 oracle (cond) "
              f"{dist(out[k], out64[k]):.3e}, |ref| max {float(np.abs(z[k]).max()):.3e}")
    for k in ("h_pret_wt", "h_pret_mt", "h_wt", "h_mt"):
        assert out[k].shape == tuple(z[k].shape)
        assert dist(out[k], z[k]) <= 1e-4, k                                                   # every row
    outside = local == 0
    assert not out["h_wt"][outside].any() and not out["h_mt"][outside].any()                   # exact zeros outside the subgraph
    for mode in ("network", "linear"):
        for k in (f"{mode}.ddg", f"{mode}.ddg_inv"):
            assert dist(out[k], z[k]) <= 1e-4 + 1e-4 * float(np.abs(z[k]).max()), k
        ref_loss = float(z[f"{mode}.loss"])
        assert abs(float(out[f"{mode}.loss"]) - ref_loss) <= 1e-4 * abs(ref_loss), mode


def test_oracle_against_reference_T1124(pret_sd, tmp_path):
    from packppi_amd.pdb_io import from_pdb_file
    z = golden("T1124")
    with gzip.open(os.path.join(GOLD, "T1124_lig.pdb.gz"), "rt") as fh:
        pdb = tmp_path / "T1124_lig.pdb"
        pdb.write_text(fh.read())
    b = as_single(mutant_data(from_pdb_file(str(pdb)), parse_mutstr(str(z["mutstr"])), ddg=0.0, log=lambda s: None))
    ap = make_random_affinity_state_dict(AFF_SEED, "network")
    with torch.no_grad():
        local = A.local_subgraph(b["X"][:, :, 1, :], b["mut_mask"])
        assert torch.equal(local, torch.from_numpy(z["local_mask"]).reshape(local.shape))
        _, ddg, inv = A.forward(ap, pret_sd, b, "network")
        _, ddg64, inv64 = A.forward(A.to_double(ap), A.to_double(pret_sd), A.to_double(b), "network")
    for k, v, v64 in (("network.ddg", ddg, ddg64), ("network.ddg_inv", inv, inv64)):
        print(f"T1124 {k}: fp32 oracle vs reference {dist(v, z[k]):.3e}, fp32 oracle vs fp64 oracle (cond) {dist(v, v64):.3e}")
        assert dist(v, z[k]) <= 1e-4 + 1e-4 * float(np.abs(z[k]).max()), k


def test_head_segments_and_padding_rows():
    """``head`` on hand-made tensors: the max is per segment of rows, padding rows count, an empty segment pools to -inf."""
    ap = make_random_affinity_state_dict(AFF_SEED, "linear")
    g = torch.Generator().manual_seed(3)
    hw, hm = torch.randn(2, 5, 128, generator=g), torch.randn(2, 5, 128, generator=g)
    ddg, inv = A.head(ap, hw, hm, [0, 5, 10])
    fwd, bwd = A.pooled(hw, hm, [0, 5, 10])
    assert torch.equal(fwd, (hm - hw).max(dim=1)[0]) and torch.equal(bwd, (hw - hm).max(dim=1)[0])
    assert torch.equal(ddg, A.ddg_predictor(ap, fwd).reshape(-1)) and torch.equal(inv, A.ddg_predictor(ap, bwd).reshape(-1))
    fwd, _ = A.pooled(hw, hm, [0, 3, 3, 10])
    assert torch.equal(fwd[0], (hm[0, :3] - hw[0, :3]).max(dim=0)[0]) and bool(torch.isneginf(fwd[1]).all())
    assert torch.equal(fwd[2], (hm.reshape(10, 128)[3:] - hw.reshape(10, 128)[3:]).max(dim=0)[0])
