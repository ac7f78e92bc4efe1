"""Container-only: run the UNMODIFIED reference PackPPI-AP (src/models/AffinityPrediction.py, SkempiDataset.prot_to_data,
skempi_datamodule.collate_fn) on seeded weights and store golden vectors.

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/make_golden_affinity.py

Writes tests/golden/g11_affinity_<case>.npz (data only).  Weights are not stored: the pretrained network is
``make_random_state_dict(WEIGHT_SEED)`` (as every other fixture), the AffinityPrediction tensors are
``make_random_affinity_state_dict(AFF_SEED, mode)``.  Stand-ins on top of refshim: a ``hydra`` module whose
``utils.instantiate`` returns its argument, ``Data.clone``, ``LightningModule.freeze``, and
``TDiffusionModule.load_from_checkpoint`` returning the seeded pretrained module (AffinityPrediction.py:42-48) -- no
reference arithmetic is restated.  Inputs are the protein dicts of g0_protein_{1BRS,2FTL}.npz and tests/golden/T1124_lig.pdb.gz
(parsed by packppi_amd.pdb_io); what the reference featurises from them is stored as well.
"""
import gzip
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refshim  # noqa: E402
from packppi_amd.batch import AFFINITY_KEYS  # noqa: E402
from packppi_amd.featurize import parse_mutstr  # noqa: E402
from packppi_amd.pdb_io import from_pdb_file  # noqa: E402
from packppi_amd.weights import make_random_affinity_state_dict, make_random_state_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 20251003          # pretrained network: the seed of every other fixture
AFF_SEED = 20261016             # AffinityPrediction's own tensors

CASES = {
    "1BRS_LA87F": ("1BRS", "LA87F", 1.25),                  # L -> F: chi1 / chi2 atoms of the wild type exist (trap 1)
    "1BRS_two_chains": ("1BRS", "SA89A,DD39A", -0.5),
    "2FTL_ignored": ("2FTL", "KI15A,RZ17A,IE189X", 2.0),    # chain Z absent, X not a residue type: both ignored
}
PADDED = ("1BRS_LA87F", "2FTL_ignored")
T1124_MUTSTR = "EA34A"


def _install_stubs():
    hy = refshim._mod("hydra")
    hy.__path__ = []
    hy.utils = refshim._mod("hydra.utils", instantiate=lambda x: x)

    def clone(self):
        return refshim.Data(**{k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in self.items()})

    refshim.Data.clone = clone

    def freeze(self):
        for p in self.parameters():
            p.requires_grad_(False)
        self.eval()

    refshim.LightningModule.freeze = freeze
    pre = refshim.build_reference_module(0)
    pre.load_state_dict(make_random_state_dict(WEIGHT_SEED), strict=True)
    import src.models.TorsionalDiffusion as TD
    TD.TDiffusionModule.load_from_checkpoint = classmethod(lambda cls, **kw: pre)


def build_ap(mode):
    from src.models.AffinityPrediction import AffinityPrediction
    m = AffinityPrediction(optimizer=None, scheduler=None, encoder_cfg=refshim.ENC, model_cfg=refshim.MDL,
                           sample_cfg=refshim.SMP, pre_checkpoint_path="seeded", mode=mode)
    own = make_random_affinity_state_dict(AFF_SEED, mode)
    missing, unexpected = m.load_state_dict(own, strict=False)
    assert not unexpected and all(k.startswith("pret.") for k in missing), (missing, unexpected)
    return m.eval()


def protein_dict(tag):
    if tag == "T1124":
        with gzip.open(os.path.join(GOLD, "T1124_lig.pdb.gz"), "rt") as fh, \
                tempfile.NamedTemporaryFile("w", suffix=".pdb", delete=False) as out:
            out.write(fh.read())
        prot = from_pdb_file(out.name)
        os.unlink(out.name)
        return prot
    z = np.load(os.path.join(GOLD, f"g0_protein_{tag}.npz"))
    return {k[5:]: z[k] for k in z.files if k.startswith("prot.")}


def ref_data(tag, mutstr, ddg):
    from src.datamodules.components.skempi_dataset import SkempiDataset
    prot = protein_dict(tag)
    arg = {k: (v.copy() if hasattr(v, "copy") else v) for k, v in prot.items()}     # prot_to_data shifts residue_index in place
    arg.update({"mutstr": mutstr, "mutations": parse_mutstr(mutstr), "pdb_path": tag, "ddG": ddg})
    return prot, SkempiDataset.prot_to_data(arg, cache_processed_data=False)


def single(d):
    """eval_affinity.py:67-72."""
    b = refshim.Data(**dict(d))
    for key in list(b.keys()):
        if not isinstance(b[key], int):
            b[key] = b[key].unsqueeze(0)
    b.num_proteins = 1
    b.max_size = b.num_nodes
    return b


def run(models, batch):
    out = {}
    with torch.no_grad():
        mt = batch.clone()
        for key in ['atom_mask', 'residue_type', 'SC_D', 'SC_D_sincos', 'SC_D_mask', 'chi_1pi_periodic_mask',
                    'chi_2pi_periodic_mask']:
            mt[key] = mt[key + '_mut']
        for mode, m in models.items():
            if mode == "network":
                out["local_mask"] = m.get_local_subgraph(batch.X[:, :, 1, :], batch.mut_mask)
                h_wt, h_mt = m.encode(batch), m.encode(mt)
                out["h_wt"], out["h_mt"] = h_wt, h_mt
                out["h_pret_wt"], out["h_pret_mt"] = m.get_pret_feature(batch), m.get_pret_feature(mt)
            else:
                h_wt, h_mt = m.get_pret_feature(batch), m.get_pret_feature(mt)
            loss, ddg = m.forward(batch)
            out[f"{mode}.ddg"] = ddg
            out[f"{mode}.ddg_inv"] = m.ddg_predictor((h_wt - h_mt).max(dim=1)[0])
            out[f"{mode}.loss"] = loss
    return out


def save(name, arrs):
    path = os.path.join(GOLD, name + ".npz")
    np.savez_compressed(path, **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in arrs.items()})
    print(f"  wrote {name}.npz  {os.path.getsize(path) / 1e6:.2f} MB", flush=True)


def main():
    torch.set_num_threads(8)
    _install_stubs()
    models = {"network": build_ap("network"), "linear": build_ap("linear")}
    keys = {mode: np.array(list(m.state_dict().keys())) for mode, m in models.items()}
    from src.datamodules.skempi_datamodule import collate_fn
    datas = {}
    for case, (tag, mutstr, ddg) in CASES.items():
        prot, d = ref_data(tag, mutstr, ddg)
        datas[case] = d
        arrs = {"prot." + k: np.asarray(prot[k]) for k in ("atom_positions", "atom_mask", "aaindex", "residue_index", "chain_id")}
        arrs.update({"mutstr": np.array(mutstr), "ddG": np.float32(ddg)})
        arrs.update({"ref." + k: d[k] for k in AFFINITY_KEYS + ("ddg",)})
        arrs.update(run(models, single(d)))
        arrs.update({f"keys.{mode}": v for mode, v in keys.items()})
        save("g11_affinity_" + case, arrs)
    b = collate_fn([datas[c] for c in PADDED])
    arrs = {"cases": np.array(PADDED)}
    arrs.update({"ref." + k: b[k] for k in AFFINITY_KEYS + ("ddg",)})
    arrs.update(run(models, b))
    save("g11_affinity_padded_B2", arrs)
    _, d = ref_data("T1124", T1124_MUTSTR, 0.0)
    out = run({"network": models["network"]}, single(d))
    save("g11_affinity_T1124", {"mutstr": np.array(T1124_MUTSTR), "local_mask": out["local_mask"],
                                "network.ddg": out["network.ddg"], "network.ddg_inv": out["network.ddg_inv"]})


if __name__ == "__main__":
    main()
