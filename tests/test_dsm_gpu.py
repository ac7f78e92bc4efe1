"""GPU checks of the denoising score-matching loss: per-row timesteps, the table-free wrapped-normal score, the loss reduction,
packed = single, the score_norm estimate and the command line, against fixtures made by the unmodified reference
(tools/oracle/make_golden_dsm.py; tests/golden/g12_dsm_*.npz).

Every figure is printed before it is asserted.  With PACKPPI_DSM_PARITY_OUT=FILE.json the measured figures are also written
there (profiles/r08_dsm_parity.json is such a record).
"""
import gzip
import json
import os

import numpy as np
import pytest
import torch

from .conftest import GOLD, load_golden

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CASES = (("L64", "g2_ops_L64"), ("B3", "g2_ops_B3"), ("T1124", "g4_T1124"))
RECORD = {}


@pytest.fixture(scope="module", autouse=True)
def _write_record():
    yield
    out = os.environ.get("PACKPPI_DSM_PARITY_OUT")
    if out and RECORD:
        with open(out, "w") as fh:
            json.dump(RECORD, fh, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def tables():
    return np.load(os.path.join(GOLD, "g12_dsm_tables.npz"))


@pytest.fixture(scope="module")
def model(weights, tables):
    from packppi_amd.module import TDiffusionModule
    return TDiffusionModule(weights, device=DEV).set_score_norm(tables["score_norm"])


def _case(tag, src):
    b, g = load_golden(src)
    z = np.load(os.path.join(GOLD, f"g12_dsm_{tag}.npz"))
    return b, g, {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" and z[k].ndim else z[k]) for k in z.files}


def _rows(b, t):
    return torch.as_tensor(t, dtype=torch.float32).repeat_interleave(b.residue_type.shape[1]).to(DEV)


# ---- per-row timesteps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g2_ops_L64", "g2_ops_B3", "packed"])
def test_constant_rows_give_pp_score_bits(name, model):
    from packppi_amd.batch import pack
    if name == "packed":
        parts = [load_golden(n) for n in ("g2_ops_L64", "g2_ops_L33")]
        b = pack([p[0] for p in parts])
        chi = torch.cat([p[1]["init_chi_seed7"] for p in parts], 1)
    else:
        b, g = load_golden(name)
        chi = g["init_chi_seed7"]
    ctx = model._context(b.to(DEV))
    for tval in (1.0, 0.5, 1.0 / 30):
        s0, h0 = ctx.score(chi, tval)
        s1, h1 = ctx.score_rows(chi, torch.full((ctx.n_rows,), tval))
        assert torch.equal(s0, s1) and torch.equal(h0, h1), tval
        s2, _ = model.network(b.to(DEV), chi.to(DEV), torch.full((ctx.n_rows,), tval))      # constant tensor: pp_score
        assert torch.equal(s0, s2)


def test_mixed_rows_equal_each_complex_alone(model):
    from packppi_amd.batch import pack, split
    # padded: g12_dsm_B3's three times, each padded row against its B = 1 batch (padding kept) at its own t
    b, g, z = _case("B3", "g2_ops_B3")
    chi = z["SC_D_noised"]
    t = z["t"]
    assert len(set(t.tolist())) == 3
    score, hV = model.network(b.to(DEV), chi.to(DEV), _rows(b, t))
    for i, one in enumerate(split(b)):
        s1, h1 = model.network(one.to(DEV), chi[i:i + 1].to(DEV), torch.full((one.residue_type.shape[1],), float(t[i])))
        assert torch.equal(score[i:i + 1], s1) and torch.equal(hV[i:i + 1], h1), i
    # packed: L64 + L33 at two times
    parts = [load_golden(n) for n in ("g2_ops_L64", "g2_ops_L33")]
    pk = pack([p[0] for p in parts]).to(DEV)
    chi = torch.cat([p[1]["init_chi_seed7"] for p in parts], 1).to(DEV)
    tt = torch.tensor([0.8125, 0.07])
    t_rows = torch.repeat_interleave(tt, torch.tensor([64, 33])).to(DEV)
    t_keep = t_rows.clone()
    score, hV = model.network(pk, chi, t_rows)
    assert torch.equal(t_rows, t_keep)                      # the caller's t is not modified
    for i, (a, e) in enumerate(((0, 64), (64, 97))):
        s1, h1 = model.network(parts[i][0].to(DEV), chi[:, a:e], torch.full((e - a,), float(tt[i])))
        assert torch.equal(score[:, a:e], s1) and torch.equal(hV[:, a:e], h1), i


@pytest.mark.parametrize("tag,src", CASES)
def test_pred_score_vs_reference(tag, src, model):
    b, g, z = _case(tag, src)
    valid = b.residue_mask.bool()
    score, _ = model.network(b.to(DEV), z["SC_D_noised"].to(DEV), _rows(b, z["t"]))
    d = (score.cpu() - z["pred_score"])[valid].abs().max().item()
    print(f"{tag}: max |pred_score - reference| {d:.3e}")
    RECORD[f"pred_score_maxabs_{tag}"] = d
    assert d < 5e-5                                          # test_network's bound


def test_nonfinite_time_is_flagged(model):
    from packppi_amd.lib import Context
    b, g = load_golden("g2_ops_L64")
    ctx = Context(model._plan, b.to(DEV))
    t = torch.full((64,), 0.5)
    ctx.score_rows(g["init_chi_seed7"], t)
    assert ctx.saturated() & 4 == 0
    t[3] = float("nan")
    ctx.score_rows(g["init_chi_seed7"], t)
    assert ctx.saturated() & 4


# ---- the wrapped-normal score ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pi_periodic", [("1pi", True), ("2pi", False)])
def test_so2_score_on_probes(name, pi_periodic, tables):
    from packppi_amd.lib import so2_grids, so2_score
    x, sigma = torch.from_numpy(tables[f"{name}.x"]).to(DEV), torch.from_numpy(tables[f"{name}.sigma"]).to(DEV)
    ref = tables[f"{name}.score"]
    score, idx = so2_score(x, sigma, pi_periodic, want_idx=True)
    score, idx = score.cpu().numpy(), idx.cpu().numpy()
    ds, dx = np.abs(idx[:, 0] - tables[f"{name}.sigma_idx"]), np.abs(idx[:, 1] - tables[f"{name}.x_idx"])
    differ = (ds > 0) | (dx > 0)
    share = float(differ.mean())
    print(f"{name}: index pairs that differ {int(differ.sum())} of {differ.size} ({100 * share:.3f} %), largest difference {int(max(ds.max(), dx.max()))}")
    ulp = np.spacing(np.abs(ref)).astype(np.float64)
    allow = np.maximum(2 * ulp, 4 * tables[f"{name}.fwd_rev"])
    err = np.abs(score.astype(np.float64) - ref.astype(np.float64))
    same = ~differ
    # ulp figure over the probes held to 2 ulp; a zero entry (sign 0, or p underflowed) has no ulp, and an entry that is rounding
    # noise of the series (x = PI: zero by symmetry) is held to its own |forward - reverse| allowance, not to its ulp
    tight = same & (ref != 0) & (allow <= 2 * ulp)
    worst_ulp = float((err[tight] / ulp[tight]).max())
    # the largest allowance beyond 2 ulp, relative to the largest |score| of its table row
    wide = same & (allow > 2 * ulp)
    rel_allow = 0.0
    if wide.any():
        k = int(np.argmax(np.where(wide, allow, 0)))
        xg, _ = so2_grids()
        row_x = torch.from_numpy(xg[0 if pi_periodic else 1].astype(np.float32)).to(DEV)
        row = so2_score(row_x, sigma[k:k + 1], pi_periodic).abs().max().item()
        rel_allow = float(allow[k] / row)
    print(f"{name}: worst error of the {int(tight.sum())} probes held to 2 ulp {worst_ulp:.2f} ulp, {int(wide.sum())} probes on the forward / reverse allowance; probes over their allowance {int((err[same] > allow[same]).sum())}; "
          f"largest allowance beyond 2 ulp relative to its row's largest |score| {rel_allow:.3e}")
    RECORD[f"so2_{name}"] = dict(index_differ_share=share, index_max_diff=int(max(ds.max(), dx.max())), worst_ulp_same_index=worst_ulp,
                                 largest_allowance_rel_row=rel_allow, probes=int(differ.size), probes_held_to_2ulp=int(tight.sum()),
                                 probes_on_forward_reverse_allowance=int(wide.sum()))
    assert max(ds.max(), dx.max()) <= 1
    assert share <= 0.005
    assert (err[same] <= allow[same]).all()


# ---- the loss -----------------------------------------------------------------------------------------------------------------------------
def _ref_num(z, b, pred):
    """The reference's own formula (TorsionalDiffusion.py:139-153) on the CPU, per protein, from the fixture's tensors."""
    sn = torch.where(b.chi_1pi_periodic_mask.bool(), z["score_norm_1pi"], z["score_norm_2pi"])
    scaled = pred * torch.sqrt(sn) * b.SC_D_mask
    return ((z["target_score"] - scaled) ** 2 / (sn + 1e-6)).sum(dim=(1, 2))


@pytest.mark.parametrize("tag,src", CASES)
def test_loss_vs_reference(tag, src, model, tables):
    b, g, z = _case(tag, src)
    gb = b.to(DEV)
    t_rows = _rows(b, z["t"])
    ctx = model._context(gb)
    sn = torch.from_numpy(tables["score_norm"]).to(DEV)
    # the reduction alone: the reference's own pred_score and target_score
    num, den = ctx.dsm_loss(z["pred_score"], z["target_score"], t_rows, sn)
    num, den = num.cpu(), den.cpu()
    r_red = ((num - z["num"]).abs() / z["num"].abs()).max().item()
    loss_red = (num.sum() / den.sum().clamp(min=1)).item()
    print(f"{tag}: reduction alone: num relative {r_red:.3e}, loss {loss_red:.12f} vs {float(z['loss']):.12f}")
    assert torch.equal(den, z["den"])
    assert r_red <= 1e-12 and abs(loss_red - float(z["loss"])) <= 1e-12 * abs(float(z["loss"]))
    # the target score from the fixture's noise
    noised, target = model.add_sc_noise_with_score(gb, t_rows, z["noise"])
    te = (target.cpu() - z["target_score"]).abs()
    off = te > 2 * torch.from_numpy(np.spacing(z["target_score"].abs().numpy()))
    share = off.float().mean().item()
    print(f"{tag}: target_score elements beyond 2 ulp {int(off.sum())} of {off.numel()} ({100 * share:.3f} %), worst {te.max().item():.3e}")
    assert share <= 0.005
    # num / loss with this project's pred_score on the fixture's noised angles and the fixture's target_score
    pred, _ = ctx.score_rows(z["SC_D_noised"], t_rows)
    num, den = ctx.dsm_loss(pred, z["target_score"], t_rows, sn)
    num, den = num.cpu(), den.cpu()
    base = _ref_num(z, b, z["pred_score"])
    allow = torch.maximum((_ref_num(z, b, z["pred_score"] + 5e-5) - base).abs(), (_ref_num(z, b, z["pred_score"] - 5e-5) - base).abs())
    diff = (num - z["num"]).abs()
    loss = (num.sum() / den.sum().clamp(min=1)).item()
    loss_allow = (allow.sum() / z["den"].sum().clamp(min=1)).item()
    print(f"{tag}: num difference {diff.tolist()} allowance {allow.tolist()}; loss {loss:.9f} vs {float(z['loss']):.9f} "
          f"(difference {abs(loss - float(z['loss'])):.3e}, allowance {loss_allow:.3e})")
    RECORD[f"loss_{tag}"] = dict(num_diff=diff.tolist(), num_allowance=allow.tolist(), loss=loss, loss_reference=float(z["loss"]),
                                 loss_diff=abs(loss - float(z["loss"])), loss_allowance=loss_allow, reduction_rel=r_red,
                                 target_beyond_2ulp_share=share)
    assert torch.equal(den, z["den"])
    assert (diff <= allow).all()
    assert abs(loss - float(z["loss"])) <= loss_allow
    # forward end to end on the padded / single batch: the same allowance
    f = model.forward(gb, t=z["t"], noise=z["noise"]).item()
    print(f"{tag}: forward {f:.9f}")
    assert abs(f - float(z["loss"])) <= loss_allow


def test_packed_equals_single(model):
    from packppi_amd.batch import pack
    parts = [load_golden(n)[0] for n in ("g2_ops_L64", "g2_ops_L33")]
    t = torch.tensor([0.3, 0.9])
    g = torch.Generator().manual_seed(11)
    noise = [torch.randn(2, n, 4, generator=g) for n in (64, 33)]
    pk = pack(parts).to(DEV)
    both = model.forward(pk, t=t, noise=torch.cat(noise, 1), per_complex=True)
    again = model.forward(pk, t=t, noise=torch.cat(noise, 1), per_complex=True)
    assert both.dtype == torch.float64 and both.shape == (2,) and torch.equal(both, again)
    for i, p in enumerate(parts):
        alone = model.forward(p.to(DEV), t=t[i:i + 1], noise=noise[i])
        assert alone.dtype == torch.float64 and alone.dim() == 0
        assert torch.equal(alone, both[i]), i
    out = model.test_step(pk)
    assert torch.isfinite(out["loss"]) and np.isfinite(model.test_loss)


def test_score_norm_tables_with_the_fixture_seed(tables):
    from packppi_amd.schedule import score_norm_tables
    mine = score_norm_tables(int(tables["np_seed"]), DEV)
    rel = np.abs(mine - tables["score_norm"]) / tables["score_norm"]
    print(f"score_norm_tables: worst relative difference {rel.max():.3e} (1pi {rel[0].max():.3e}, 2pi {rel[1].max():.3e}), median {np.median(rel):.3e}")
    RECORD["score_norm_tables_worst_rel"] = float(rel.max())
    assert mine.dtype == np.float64 and mine.shape == (2, 5001)
    assert rel.max() <= 1e-3


def test_cli_end_to_end(tmp_path, weights, tables, capsys):
    from packppi_amd.cli import test_diffusion as cli
    from packppi_amd.module import TDiffusionModule
    pdb = tmp_path / "T1124_lig.pdb"
    with gzip.open(os.path.join(GOLD, "T1124_lig.pdb.gz"), "rb") as src, open(pdb, "wb") as dst:
        dst.write(src.read())
    ckpt, sn = tmp_path / "model.ckpt", tmp_path / "score_norm.npy"
    torch.save({"state_dict": weights}, ckpt)
    np.save(sn, tables["score_norm"])
    cli.main(["--input", str(pdb), "--ckpt_path", str(ckpt), "--config_dir", os.path.join(GOLD, "configs"), "--seed", "5",
              "--score_norm", str(sn), "--device", DEV])
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if ln.startswith("test/loss")]
    assert len(line) == 1, out
    printed = float(line[0].split()[1])
    model = TDiffusionModule(weights, device=DEV).set_score_norm(str(sn))
    want = cli.test_loss(model, cli.packed_inputs([str(pdb)], DEV), seed=5).mean().item()
    print(f"cli test/loss {printed:.6f}, forward with the same seed {want:.9f}")
    assert np.isfinite(printed) and f"{want:.6f}" == line[0].split()[1]
    assert str(pdb) in out
