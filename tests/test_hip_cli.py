"""GPU: the two command-line entry points end to end (PDB in -> structure.pdb out), and the multi-complex sharding path."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pdb_file(tmp_path_factory):
    from packppi_amd import synth
    from packppi_amd.pdb_io import to_pdb
    d = tmp_path_factory.mktemp("cli")
    p = d / "complex.pdb"
    p.write_text(to_pdb(synth.make_complex(60, 21)))
    return p


def test_eval_diffusion_cli(pdb_file, tmp_path, capsys):
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.pdb_io import from_pdb_file
    out = tmp_path / "out"
    eval_diffusion.main(["--input", str(pdb_file), "--outdir", str(out), "--molprobity_clash_loc", "/nonexistent",
                         "--device", "cuda", "--random_weights", "3", "--steps", "10", "--seed", "5", "--use_proximal"])
    text = capsys.readouterr().out
    assert "----- Metric: -----" in text and "atom_rmsd" in text and "----- Finishing evaluation! -----" in text
    assert (out / "structure.pdb").exists()
    a, b = from_pdb_file(pdb_file), from_pdb_file(out / "structure.pdb")
    assert np.array_equal(a["aaindex"], b["aaindex"]) and np.array_equal(a["atom_mask"], b["atom_mask"])
    bb = np.abs(a["atom_positions"][:, :4] - b["atom_positions"][:, :4])
    assert np.nanmax(bb) < 1.1e-3            # backbone is copied through (3-decimal PDB rounding)


class _FakeOmegaConf(dict):
    """Stands in for omegaconf.DictConfig / a Lightning callback inside a pickled checkpoint; un-importable when it is read."""


def _write_lightning_ckpt(path, weights):
    """A Lightning-format .ckpt: state_dict + hyper_parameters and callbacks whose classes this image cannot import."""
    import sys
    import types
    fake = types.ModuleType("omegaconf_fake_pkg")
    fake.DictConfig = _FakeOmegaConf
    old = (_FakeOmegaConf.__module__, _FakeOmegaConf.__qualname__, _FakeOmegaConf.__name__)
    _FakeOmegaConf.__module__, _FakeOmegaConf.__qualname__, _FakeOmegaConf.__name__ = "omegaconf_fake_pkg", "DictConfig", "DictConfig"
    sys.modules["omegaconf_fake_pkg"] = fake
    try:
        sd = dict(weights)
        sd["train_loss.mean_value"] = torch.zeros(())             # metric buffers ride along in real checkpoints (strict=False)
        torch.save({"state_dict": sd, "epoch": 3, "global_step": 1234, "pytorch-lightning_version": "2.0.0",
                    "hyper_parameters": {"encoder_cfg": _FakeOmegaConf(node_in=35), "model_cfg": _FakeOmegaConf(hidden_dim=128),
                                         "sample_cfg": _FakeOmegaConf(mode="ode")},
                    "callbacks": {"ModelCheckpoint{'monitor': 'val/loss'}": _FakeOmegaConf(best_model_score=torch.tensor(0.1))},
                    "optimizer_states": [], "lr_schedulers": []}, path)
    finally:
        del sys.modules["omegaconf_fake_pkg"]
        _FakeOmegaConf.__module__, _FakeOmegaConf.__qualname__, _FakeOmegaConf.__name__ = old


def test_checkpoint_file_to_structure_pdb(pdb_file, tmp_path, capsys, weights, monkeypatch):
    """f3 end to end: a Lightning-format .ckpt FILE and a configs/ tree -> cli.eval_diffusion -> OUTDIR/structure.pdb, held to the
    oracle (eval_diffusion.py:22-82).  The tree's Sampling.yaml asks for annealed_temp 2.5 (not the default 3) and its
    eval_diffusion.yaml names the checkpoint; the initial noise is pinned (add_sc_noise replaced by the oracle's seeded draw);
    the written side-chain coordinates must be the oracle's atom14 coordinates at the PDB format's 3 decimals."""
    from oracle import ref_cpu as O
    from packppi_amd.analysis import ProteinAnalysis
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.pdb_io import from_pdb_file
    from .test_host import _write_config_tree
    ckpt = tmp_path / "PackPPI_pretrain_last.ckpt"
    _write_lightning_ckpt(ckpt, weights)
    tree = _write_config_tree(tmp_path / "configs", sample_cfg=dict(annealed_temp=2.5), top=dict(ckpt_path=str(ckpt)))
    b = ProteinAnalysis(None, str(tmp_path / "w"), "cpu").get_prot(str(pdb_file))
    init = O.add_sc_noise(b, torch.ones(b.max_size), O.initial_noise(b, torch.Generator().manual_seed(11)))
    monkeypatch.setattr(TDiffusionModule, "add_sc_noise", lambda self, batch, t: (init.to(self.device), None))
    out = tmp_path / "out"
    eval_diffusion.main(["--input", str(pdb_file), "--outdir", str(out), "--molprobity_clash_loc", "/nonexistent",
                         "--device", "cuda", "--config_dir", str(tree), "--steps", "10"])
    text = capsys.readouterr().out
    assert f"Loading {ckpt} checkpoint" in text and "----- Metric: -----" in text
    monkeypatch.setattr(O, "ANNEALED_TEMP", 2.5)
    chi = O.sampling(weights, b, init, torch.linspace(1, 0, 11))
    want = O.atom14_coords(b.X, b.residue_type, b.BB_D, chi)[0].numpy()
    got = from_pdb_file(out / "structure.pdb")
    mask = got["atom_mask"].astype(bool)
    assert np.array_equal(mask, b.atom_mask[0].numpy().astype(bool))
    d = np.abs(got["atom_positions"] - want)[mask]
    assert d.max() < 5e-4 + 2e-4, d.max()          # half a unit of the third decimal + the 1e-4 rad tolerance on a ~3 A lever arm
    # annealed_temp from the YAML did reach the kernels: the default (3) gives other coordinates
    monkeypatch.setattr(O, "ANNEALED_TEMP", 3.0)
    other = O.atom14_coords(b.X, b.residue_type, b.BB_D, O.sampling(weights, b, init, torch.linspace(1, 0, 11)))[0].numpy()
    assert np.abs(other - want)[mask].max() > 1e-2
    # a tree asking for another architecture is refused with the key in the message
    bad = _write_config_tree(tmp_path / "configs_bad", model_cfg=dict(hidden_dim=256), top=dict(ckpt_path=str(ckpt)))
    with pytest.raises(RuntimeError, match=r"model_cfg\.hidden_dim = 256"):
        eval_diffusion.main(["--input", str(pdb_file), "--outdir", str(out), "--molprobity_clash_loc", "/nonexistent",
                             "--device", "cuda", "--config_dir", str(bad), "--steps", "2"])


def test_proximal_optimize_cli(pdb_file, tmp_path, capsys):
    from packppi_amd.cli import proximal_optimize
    out = tmp_path / "out2"
    proximal_optimize.main(["--input", str(pdb_file), "--outdir", str(out), "--molprobity_clash_loc", "/nonexistent",
                            "--num_steps", "10", "--clash_overlap_tolerance", "0.1"])
    text = capsys.readouterr().out
    assert "----- Starting optimize! -----" in text and "----- Finishing optimize! -----" in text
    assert (out / "structure.pdb").exists()


def test_sample_sharded_single_rank(weights):
    """parallel.sample_sharded without a process group: every complex handled locally, rows sorted by id."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    from packppi_amd.module import TDiffusionModule
    from packppi_amd.parallel import METRIC_KEYS, sample_sharded
    m = TDiffusionModule(weights, device="cuda:0")
    m.schedule = torch.linspace(1, 0, 6)
    cs = [protein_to_batch(synth.make_complex(n, 70 + n)).to("cuda:0") for n in (30, 44, 36)]
    torch.manual_seed(0)
    chis, ids, rows = sample_sharded(m, cs)
    assert ids.tolist() == [0, 1, 2] and rows.shape == (3, len(METRIC_KEYS)) and torch.isfinite(rows).all()
    assert set(chis) == {0, 1, 2} and chis[1].shape == (1, 44, 4)


def test_padded_batch_equals_per_complex(weights):
    """B=3 padded batch through one ctx == each complex on its own (complexes are independent)."""
    from packppi_amd import synth
    from packppi_amd.batch import collate
    from packppi_amd.featurize import protein_to_data
    from packppi_amd.batch import as_single
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device="cuda:0")
    ds = [protein_to_data(synth.make_complex(n, 90 + n)) for n in (40, 52, 33)]
    b = collate(ds).to("cuda:0")
    sched = torch.linspace(1, 0, 8)
    g = torch.Generator().manual_seed(4)
    init = (torch.rand(3, 52, 4, generator=g) * 2 - 1) * 3.0 * b.SC_D_mask.cpu()
    joint = m._context(b).sample(init.to("cuda:0"), sched).cpu()
    for i, d in enumerate(ds):
        bi = as_single(d).to("cuda:0")
        L = d.num_nodes
        solo = m._context(bi).sample(init[i:i + 1, :L].to("cuda:0"), sched).cpu()
        assert (joint[i, :L] - solo[0]).abs().max() < 2e-5
        assert float(joint[i, L:].abs().sum()) == 0.0


def test_get_metric_matches_reference(tmp_path):
    """ProteinAnalysis.get_metric on a written true / predicted pair vs the reference's own get_metric on the same files
    (protein_analysis.py:36-91; fixture tools/oracle/make_golden_io.py: chi recomputed from the 3-decimal files, accuracies,
    interface accuracy, atom_rmsd; the clashscore is an external MolProbity call, a constant on both sides)."""
    import os
    import numpy as np
    from packppi_amd.analysis import ProteinAnalysis
    from packppi_amd.pdb_io import to_pdb
    gold = os.path.join(os.path.dirname(__file__), "golden")
    z = np.load(os.path.join(gold, "g8_io.npz"))
    g0 = np.load(os.path.join(gold, "g0_protein_1BRS.npz"))
    prot = {k[5:]: g0[k] for k in g0.files if k.startswith("prot.")}
    pred = dict(prot, atom_positions=z["pred.atom_positions"])
    (tmp_path / "true.pdb").write_text(to_pdb(prot))
    (tmp_path / "pred.pdb").write_text(to_pdb(pred))
    pa = ProteinAnalysis(None, str(tmp_path / "work"), device="cuda:0")
    pa.get_clashscore = lambda pdb: 12.34
    m = pa.get_metric(str(tmp_path / "true.pdb"), str(tmp_path / "pred.pdb"))
    keys = [k[7:] for k in z.files if k.startswith("metric.")]
    assert sorted(m) == sorted(keys)
    for k in keys:
        assert abs(float(m[k]) - float(z["metric." + k])) < 2e-5 * max(1.0, abs(float(z["metric." + k]))), (k, float(m[k]))


@pytest.mark.parametrize("workload,rows", [(None, 256), ("t1124", 2)])
def test_bench_two_ranks_as_the_driver_launches_it(workload, rows):
    """The driver's multi-GPU command line, rehearsed: `python bench.py --gpus 2 --steps K --warmup W` -- NO --workload, as the
    driver starts it -- as a FRESH child process (it spawns torch.distributed.run itself before anything touches the GPU), two
    ranks sharing this box's one GPU over gloo (BENCH_DIST_BACKEND; on a multi-GPU node the backend is "nccl" = RCCL and nothing
    else differs).  The default at N > 1 is BASELINE configs[4]: the 256 complexes sharded over the ranks, metric rows gathered
    inside the timed pass, "strong" scaling, one T1124 replica per rank as `secondary`; `--workload t1124` stays available.  One
    JSON line whose last key is `summary`, both ranks seen, every metric row gathered, exit code 0."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BENCH_DIST_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PACKPPI_LIB"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0", "--full"]
                       + (["--workload", workload, "--no-secondary"] if workload else []),
                       env=env, cwd=root, capture_output=True, text=True, timeout=1100)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["ranks_seen"] == 2 and out["metrics_rows_gathered"] == rows
    assert out["value"] > 0 and out["scaling"] == ("weak" if workload == "t1124" else "strong")
    assert list(out)[-1] == "summary" and len(json.dumps(out["summary"])) < 1500
    if workload == "t1124":
        assert out["parity"]["max_abs_dchi_vs_reference_rad"] < 1e-4
    else:
        assert out["config"]["complexes_total"] == 256
        assert "configs[4]" in out["config"]["workload"]
        rep = [e for e in out["secondary"] if e["config"] == "configs[1] replicas"]
        assert len(rep) == 1 and rep[0]["scaling"] == "weak" and rep[0]["max_abs_dchi_vs_reference_rad"] < 1e-4
        assert "c4_sharded" in out["summary"]["cfg"] and "c1_replicas" in out["summary"]["cfg"]


def test_bench_one_rank_through_rccl():
    """The collectives of the multi-GPU path on the backend the driver's runs use: `torch.distributed.run --nproc-per-node 1
    bench.py --gpus 1 --workload c5` gives the rank a process group of one with backend "nccl" (= RCCL), so the communicator
    is created on this GPU and the fences' barriers, the max-over-ranks all-reduce and the metric all-gather of
    parallel.gather_metric_rows (int64 id block + float32 rows, device tensors) run as RCCL kernels.  A fresh child process;
    what a second GPU adds is the transport, not the calls."""
    import json
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PACKPPI_LIB", "BENCH_DIST_BACKEND", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "1", "--warmup", "0",
                        "--full", "--cpu-steps", "0", "--no-secondary", "--workload", "c5"],
                       env=env, cwd=root, capture_output=True, text=True, timeout=900)
    if r.returncode != 0 and any(k in r.stderr for k in ("ncclSystemError", "ncclInternalError", "unhandled system error",
                                                          "ncclUnhandledCudaError", "NCCL WARN")) and "Traceback" in r.stderr \
            and "packppi_amd" not in r.stderr.split("Traceback")[-1]:
        pytest.skip("RCCL could not create a communicator on this box (not this package's code): " + r.stderr[-300:])
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["dist_backend"] == "nccl" and out["n_gpus"] == 1 and out["ranks_seen"] == 1
    assert out["metrics_rows_gathered"] == 256 and out["value"] > 0


def test_bench_plain_run_and_dump_outputs(tmp_path):
    """`python bench.py --gpus 1 --steps K --warmup W --dump-outputs DIR` as the driver runs it: a fresh child process, the
    headline line only (none of the --full parts), K timed steps, and DIR/chi.npy = the angles the last timed step returned --
    float32, the T1124 fixture's shape, within 1e-4 rad of the reference's 100-step output on the same noise."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PACKPPI_LIB", "TORCHELASTIC_RUN_ID"):
        env.pop(k, None)
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out_dir)], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-2500:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    out = json.loads(lines[0])
    assert out["steps"] == 2 and out["warmup"] == 1 and out["ms_per_step"] > 0 and out["higher_is_better"] is True
    assert out["metric"] == "sampled residues/sec at 100 diffusion steps" and out["unit"] == "residues/s" and out["dtype"].startswith("f32")
    assert abs(out["value"] - 738 * 1e3 / out["ms_per_step"]) < 1e-6 * out["value"]
    assert not {"secondary", "roofline", "cpu_baseline", "parity"} & set(out) and list(out)[-1] == "summary"
    assert sorted(os.listdir(out_dir)) == ["chi.npy"]
    chi = np.load(out_dir / "chi.npy")
    z = np.load(os.path.join(root, "tests", "golden", "g4_T1124.npz"))
    assert chi.dtype == np.float32 and chi.shape == z["chi_ode_100"].shape
    d = torch.from_numpy(chi).double() - torch.from_numpy(z["chi_ode_100"]).double()
    d = torch.minimum(d.abs(), (2 * np.pi - d.abs()).abs())[torch.from_numpy(z["batch.SC_D_mask"]).bool()]
    assert float(d.max()) < 1e-4, float(d.max())
