"""PackPPI-AP on the MI355X against the unmodified reference (tests/golden/g11_affinity_*.npz; weights: the seeded
make_random_state_dict / make_random_affinity_state_dict of tools/oracle/make_golden_affinity.py)."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from packppi_amd.affinity import AffinityPrediction
from packppi_amd.batch import as_single, collate_affinity
from packppi_amd.featurize import mutant_data, parse_mutstr
from packppi_amd.weights import make_random_affinity_state_dict, make_random_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED, AFF_SEED = 20251003, 20261016
CASES = ("1BRS_LA87F", "1BRS_two_chains", "2FTL_ignored")
DEV = "cuda:0"


def golden(case):
    return np.load(os.path.join(GOLD, f"g11_affinity_{case}.npz"))


def case_data(case):
    z = golden(case)
    p = {k[5:]: z[k] for k in z.files if k.startswith("prot.")}
    return mutant_data(p, parse_mutstr(str(z["mutstr"])), ddg=float(z["ddG"]), log=lambda s: None)


_models = {}


def model(mode):
    if mode not in _models:
        _models[mode] = AffinityPrediction(make_random_affinity_state_dict(AFF_SEED, mode), make_random_state_dict(WEIGHT_SEED),
                                           mode=mode, device=DEV)
    return _models[mode]


def close(a, ref, atol=1e-4, rtol=0.0):
    a = a.detach().float().cpu().reshape(ref.shape)
    ref = torch.as_tensor(ref).float()
    err = (a - ref).abs().max().item()
    assert err <= atol + rtol * ref.abs().max().item(), err


def batch_of(case):
    if case == "padded_B2":
        z = golden(case)
        return collate_affinity([case_data(str(c)) for c in z["cases"]]).to(DEV)
    return as_single(case_data(case)).to(DEV)


@pytest.mark.parametrize("mode", ["network", "linear"])
@pytest.mark.parametrize("case", CASES + ("padded_B2",))
def test_forward_against_reference(case, mode):
    z = golden(case)
    m = model(mode)
    b = batch_of(case)
    loss, ddg = m.forward(b)
    close(ddg, z[f"{mode}.ddg"], 1e-4, 1e-4)
    close(m.last_ddg_inv, z[f"{mode}.ddg_inv"], 1e-4, 1e-4)
    ref_loss = float(z[f"{mode}.loss"])
    assert abs(loss.item() - ref_loss) <= 1e-4 * abs(ref_loss)
    assert m.saturated() == 0
    if mode == "network":
        from packppi_amd.affinity import mutant_view
        close(m.get_pret_feature(b), z["h_pret_wt"])
        close(m.get_pret_feature(mutant_view(b)), z["h_pret_mt"])
        close(m.encode(b), z["h_wt"])
        h_mt = m.encode(mutant_view(b))
        close(h_mt, z["h_mt"])
        outside = torch.from_numpy(z["local_mask"]).to(DEV).reshape(h_mt.shape[:2]) == 0
        assert not h_mt[outside].any()          # rows outside the subgraph are exact zeros


@pytest.mark.parametrize("mode", ["network", "linear"])
def test_predict_many_bitwise_equals_single_runs(mode):
    m = model(mode)
    singles = []
    for c in CASES:
        _, d = m.forward(batch_of(c))
        singles.append(d.reshape(-1))
    ddg, _ = m.predict_many([case_data(c) for c in CASES])
    assert m.saturated() == 0
    assert torch.equal(ddg.cpu(), torch.cat(singles).cpu())


def test_mutation_branch_independent_of_tie_rule():
    m = model("network")
    out = {}
    for ties in ("lower_index", "aten_cpu"):
        m.set_mutation_knn_ties(ties)
        out[ties] = [m.encode(batch_of(c)).cpu() for c in CASES + ("padded_B2",)]
    m.set_mutation_knn_ties("aten_cpu")
    for a, b in zip(out["lower_index"], out["aten_cpu"]):
        assert torch.equal(a, b)


def _run_cli(tmp_path, *extra):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    with gzip.open(os.path.join(GOLD, "T1124_lig.pdb.gz"), "rt") as fh:
        pdb = tmp_path / "T1124_lig.pdb"
        pdb.write_text(fh.read())
    cmd = [sys.executable, "-m", "packppi_amd.cli.eval_affinity", "--input", str(pdb), "--device", DEV, *extra]
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


def _checkpoints(tmp_path):
    pre = make_random_state_dict(WEIGHT_SEED)
    torch.save({"state_dict": pre}, tmp_path / "pre.ckpt")
    own = make_random_affinity_state_dict(AFF_SEED, "network")
    # the AP checkpoint's pret.* tensors override the pre-checkpoint's: a perturbed pre-checkpoint must not matter
    torch.save({"state_dict": {k: v + 1.0 for k, v in pre.items()}}, tmp_path / "pre_other.ckpt")
    sd = dict(own)
    sd.update({"pret." + k: v for k, v in pre.items()})
    torch.save({"state_dict": sd, "hyper_parameters": {"mode": "network"}}, tmp_path / "ap.ckpt")
    return tmp_path / "ap.ckpt", tmp_path / "pre_other.ckpt"


def _values(out):
    return [float(ln.split(" is ")[1].split()[0]) for ln in out.splitlines() if "predicted binding affinity change" in ln]


def test_cli_t1124_matches_reference(tmp_path):
    ap, pre = _checkpoints(tmp_path)
    z = golden("T1124")
    out = _run_cli(tmp_path, "--mutstr", str(z["mutstr"]), "--ckpt_path", str(ap), "--pre_ckpt_path", str(pre))
    (v,) = _values(out)
    ref = float(z["network.ddg"].reshape(-1)[0])
    assert abs(v - ref) <= 1e-4 + 1e-4 * abs(ref) + 5e-5, (v, ref)      # + half a unit of the printed 4th decimal
    assert "----- The predicted binding affinity change (wildtype-mutant) is" in out


def test_cli_mutlist_matches_single_runs(tmp_path):
    ap, pre = _checkpoints(tmp_path)
    sets = ["EA34A", "RA35A,LA36A", "EB34A"]
    (tmp_path / "sets.txt").write_text("\n".join(sets) + "\n")
    ck = ["--ckpt_path", str(ap), "--pre_ckpt_path", str(pre)]
    many = _values(_run_cli(tmp_path, "--mutlist", str(tmp_path / "sets.txt"), *ck))
    singles = [_values(_run_cli(tmp_path, "--mutstr", s, *ck))[0] for s in sets]
    assert many == singles


def test_missing_checkpoint_key_is_named(tmp_path):
    pre = make_random_state_dict(WEIGHT_SEED)
    own = make_random_affinity_state_dict(AFF_SEED)
    del own["ddg_predictor.4.bias"]
    torch.save({"state_dict": own, "hyper_parameters": {"mode": "network"}}, tmp_path / "ap.ckpt")
    torch.save({"state_dict": pre}, tmp_path / "pre.ckpt")
    with pytest.raises(RuntimeError, match="ddg_predictor.4.bias"):
        AffinityPrediction.load_from_checkpoint(str(tmp_path / "ap.ckpt"), pre_checkpoint_path=str(tmp_path / "pre.ckpt"),
                                                map_location=DEV)
