"""Decoy ensembles on the device (csrc/pp_ensemble.hip).

What is held: a decoy is bit for bit the complex sampled alone under its decoy key (sde and ode, with and without the proximal
stage); pp_ensemble_reduce against an fp64 NumPy restatement of its header comment; its edges (one decoy, cancelling decoys, ties),
its independence of what else is packed, its refusals, and the command line.

Complexes as in tests/test_seeded_noise.py: L = 33 (the smallest K = 32 complex, one row past two 16-row tiles) and L = 40, a 4-point
schedule.  The reduced batch is 5 decoys of each, N = 365: the L = 33 decoys (132 elements) leave lanes of the 256-thread workgroup
idle, the L = 40 ones (160 elements) too; the consensus launch has two workgroups (4 * 73 = 292 lanes)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = 0x1234_5678_9abc_def0
KEYS = (7, 2 ** 40 + 3)
LENS = (33, 40)
SCHED = torch.linspace(1, 0, 4)
D = 5
# half an fp32 ulp at pi (1.2e-7) for the stored mean, plus margin for the device's and NumPy's fp64 sin / cos / atan2
MEAN_TOL = 5e-7


@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = SCHED
    return m


@pytest.fixture(scope="module")
def complexes():
    """L33 and L40 on the device, each carrying its key both ways (``complex_key`` for pack(), ``complex_keys`` for sampling())."""
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    cs = [protein_to_batch(synth.make_complex(n, 70 + n)).to(DEV) for n in LENS]
    for c, k in zip(cs, KEYS):
        c["complex_key"] = k
        c["complex_keys"] = [k]
    return cs


def _solo(c, key):
    s = type(c)({k: v for k, v in c.items() if not k.startswith("complex_key")})
    s["complex_keys"] = [key]
    return s


def _ctx(model, batch):
    from packppi_amd.lib import Context
    return Context(model._plan, batch)


@pytest.fixture(scope="module")
def two_groups(model, complexes):
    """5 seeded decoys of L33 and of L40 in one packed batch (N = 365), their angles, a context, the per-residue clash and the two
    reductions: computed once, shared, never modified."""
    from packppi_amd.batch import replicate_many
    pb = replicate_many(complexes, D)
    assert pb.max_size == 365 and pb.n_groups == 2
    chi = model.sampling(pb, seed=SEED)
    ctx = _ctx(model, pb)
    per_res = ctx.clash(chi)
    return dict(pb=pb, chi=chi, ctx=ctx, per_res=per_res, clash=ctx.ensemble_reduce(chi, D, per_res=per_res, select="clash"),
                medoid=ctx.ensemble_reduce(chi, D, per_res=per_res, select="medoid"))


# ---- the header comment of csrc/pp_ensemble.hip, restated in NumPy fp64 ------------------------------------------------------------
def consensus64(chi, mask, m1pi, offs, n_dec):
    """(mean, resultant) fp64 [N / D, 4] from chi [N, 4]: d = 0 .. D - 1 in order, p = 2 on the pi-periodic entries."""
    chi, means, res = np.asarray(chi, dtype=np.float64), [], []
    for g in range((len(offs) - 1) // n_dec):
        a0, b0 = offs[g * n_dec], offs[g * n_dec + 1]
        p = np.where(m1pi[a0:b0], 2.0, 1.0)
        S, Cc = np.zeros((b0 - a0, 4)), np.zeros((b0 - a0, 4))
        for d in range(n_dec):
            a = offs[g * n_dec + d]
            S = S + np.sin(p * chi[a:a + b0 - a0])
            Cc = Cc + np.cos(p * chi[a:a + b0 - a0])
        valid = mask[a0:b0] != 0
        means.append(np.where(valid, np.arctan2(S, Cc) / p, 0.0))
        res.append(np.where(valid, np.sqrt(S * S + Cc * Cc) / n_dec, 0.0))
    return np.concatenate(means), np.concatenate(res)


def scores64(chi, mean32, mask, m1pi, per_res, offs, n_dec):
    """(dev, clash) fp64 [B] from the device's STORED fp32 mean: delta wrapped into [-P / 2, P / 2), P = 2 pi / p."""
    chi, mean = np.asarray(chi, dtype=np.float64), np.asarray(mean32, dtype=np.float64)
    dev, clash = [], []
    for s in range(len(offs) - 1):
        a, b = offs[s], offs[s + 1]
        base = offs[(s // n_dec) * n_dec] // n_dec
        P = np.where(m1pi[a:b], np.pi, 2.0 * np.pi)
        dl = chi[a:b] - mean[base:base + b - a]
        dl = dl - P * np.floor((dl + P / 2.0) / P)
        m = mask[a:b].astype(np.float64)
        dev.append(np.sqrt((dl * dl * m).sum() / max(m.sum(), 1.0)))
        clash.append(np.asarray(per_res[a:b], dtype=np.float64).sum() / (b - a))
    return np.array(dev), np.array(clash)


def _host(pb):
    return (pb.SC_D_mask[0].cpu().numpy(), pb.chi_1pi_periodic_mask[0].cpu().numpy().astype(bool), pb.seg_offsets_host)


def _wrapped(d, P):
    return np.abs(d - P * np.round(d / P))


# ---- 1. a decoy is the complex alone ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["sde", "ode"])
def test_a_decoy_is_the_complex_alone(mode, model, complexes):
    """Decoy d of the key-7 complex == sampling(seed=) of that complex alone under decoy_key(7, d); decoy 0 == today's sampling.  In
    ode mode only the initial noise differs between decoys."""
    from packppi_amd.batch import decoy_key, unpack
    c = complexes[0]
    model.hparams.sample_cfg.mode = mode
    try:
        out = model.sample_ensemble(c, 3, seed=SEED, select=None, return_all=True)
        chi, pb = out["decoys"]
        assert out["keys"] == [decoy_key(7, d) for d in range(3)] and pb.seg_offsets_host == [0, 33, 66, 99]
        parts = unpack(pb, chi)
        for d in range(3):
            alone = model.sampling(_solo(c, decoy_key(7, d)), seed=SEED)
            assert torch.isfinite(alone).all() and torch.equal(parts[d], alone), d
        assert torch.equal(parts[0], model.sampling(c, seed=SEED))
        for i, j in ((0, 1), (0, 2), (1, 2)):
            assert not torch.equal(parts[i], parts[j])
        assert out["best"].tolist() == [0] and torch.equal(out["selected"], parts[0])           # select=None: decoy 0
        assert torch.equal(model.sample_ensemble(c, 3, seed=SEED, select=None), parts[0])
    finally:
        model.hparams.sample_cfg.mode = "ode"


# ---- 2. the reduction against fp64 -----------------------------------------------------------------------------------------------
def test_reduce_against_fp64(two_groups):
    t = two_groups
    pb, chi = t["pb"], t["chi"][0].cpu().numpy()
    mask, m1pi, offs = _host(pb)
    valid = mask != 0
    mean_ref, res_ref = consensus64(chi, mask, m1pi, offs, D)
    cons_valid = np.concatenate([valid[0:33], valid[165:205]])
    cons_m1pi = np.concatenate([m1pi[0:33], m1pi[165:205]])
    assert cons_valid.sum() > 100 and (~cons_valid).sum() > 0 and cons_m1pi[cons_valid].any() and (~cons_m1pi[cons_valid]).any()
    for name in ("clash", "medoid"):
        r = t[name]
        mean, res = r.mean[0].cpu().numpy(), r.resultant[0].cpu().numpy()
        assert mean.shape == (73, 4) and mean.dtype == np.float32
        # mean: wrapped on its period, where the direction is defined (reference resultant >= 1e-6); nothing may be left out here
        cmp = cons_valid & (res_ref >= 1e-6)
        left_out = int((cons_valid & ~cmp).sum())
        print(f"{name}: {left_out} of {int(cons_valid.sum())} valid entries left out of the mean comparison")
        assert left_out <= 0.01 * cons_valid.sum() and left_out == 0
        P = np.where(cons_m1pi, np.pi, 2.0 * np.pi)
        dm = _wrapped(mean.astype(np.float64) - mean_ref, P)[cmp].max()
        dr = np.abs(res.astype(np.float64) - res_ref)[cons_valid].max()
        print(f"{name}: max |mean - ref| {dm:.3e} rad, max |resultant - ref| {dr:.3e}")
        assert dm <= MEAN_TOL and dr <= 1e-6
        assert (res[cons_valid] >= 0).all() and (res[cons_valid] <= 1 + 1e-6).all() and res[cons_valid].min() < 0.99
        assert (mean[~cons_valid] == 0).all() and (res[~cons_valid] == 0).all()                  # masked entries
        # dev, clash: fp64 sums of the same inputs (the device's stored mean, the same per_res), only the order differs
        dev_ref, clash_ref = scores64(chi, mean, mask, m1pi, t["per_res"].reshape(-1).cpu().numpy(), offs, D)
        dev, clash = r.dev.cpu().numpy(), r.clash.cpu().numpy()
        assert dev.dtype == np.float64 and dev.shape == (10,) and (dev > 0).all()
        print(f"{name}: dev {dev}, clash {clash}")
        assert np.all(np.abs(dev - dev_ref) <= 1e-9 * np.abs(dev_ref) + 1e-12)
        assert np.all(np.abs(clash - clash_ref) <= 1e-9 * np.abs(clash_ref) + 1e-12)
        # selection: the lowest-index argmin of the RETURNED scores, and that decoy's rows bit for bit
        score = clash if name == "clash" else dev
        best = r.best.cpu().tolist()
        assert best == [int(np.argmin(score[g * D:(g + 1) * D])) for g in range(2)]
        rows = [t["chi"][0, offs[g * D + best[g]]:offs[g * D + best[g] + 1]] for g in range(2)]
        assert torch.equal(r.chi_best[0], torch.cat(rows))
    assert torch.equal(t["clash"].mean, t["medoid"].mean) and torch.equal(t["clash"].dev, t["medoid"].dev)
    r0 = t["ctx"].ensemble_reduce(t["chi"], D, want_best=False)                                    # no per_res, no selection
    assert r0.clash is None and r0.chi_best is None and r0.best.tolist() == [0, 0] and torch.equal(r0.dev, t["clash"].dev)


# ---- 3. edges --------------------------------------------------------------------------------------------------------------------
def test_one_decoy(model, complexes, two_groups):
    """D = 1, on the plain B = 1 batch and on the packed copy of it: resultant 1, best 0, mean = the angle modulo its period.  dev is
    the RMS of x - (the fp32 mean): 0 up to the rounding of the stored mean where a pi-periodic angle lies outside [-pi/2, pi/2] --
    half an fp32 ulp below pi/2, 6e-8 -- so it is held to 6.1e-8, not to exact 0 (measured on the MI355X: 8.0e-9)."""
    from packppi_amd.batch import replicate
    c = complexes[0]
    chi = two_groups["chi"][:, 33:66].clone()                             # decoy 1 of L33: sampled angles in [-pi, pi)
    valid = (c.SC_D_mask[0] != 0).cpu().numpy()
    m1pi = c.chi_1pi_periodic_mask[0].cpu().numpy().astype(bool)
    r0, c0 = np.argwhere(valid & m1pi)[0]
    chi[0, r0, c0] = 2.0                                                  # a pi-periodic angle beyond pi / 2, whatever was sampled
    x = chi[0].cpu().numpy().astype(np.float64)
    assert (np.abs(x[valid & m1pi]) > np.pi / 2).any()                    # the modulo is exercised
    for batch in (c, replicate(c, 1)):
        ctx = _ctx(model, batch)
        r = ctx.ensemble_reduce(chi, 1, per_res=ctx.clash(chi), select="clash")
        res, mean = r.resultant[0].cpu().numpy(), r.mean[0].cpu().numpy().astype(np.float64)
        assert np.abs(res[valid] - 1).max() <= 1e-6 and (res[~valid] == 0).all()
        P = np.where(m1pi, np.pi, 2 * np.pi)
        assert _wrapped(mean - x, P)[valid].max() <= MEAN_TOL
        assert (np.abs(mean[valid]) <= P[valid] / 2 + MEAN_TOL).all()
        print("D = 1: dev", r.dev.tolist())
        assert r.dev.shape == (1,) and 0 <= float(r.dev[0]) <= 6.1e-8
        assert r.best.tolist() == [0] and torch.equal(r.chi_best, chi)


def test_cancelling_and_identical_decoys(model, complexes, two_groups):
    from packppi_amd.batch import replicate
    c = complexes[0]
    pb = replicate(c, 2)
    ctx = _ctx(model, pb)
    chi0 = two_groups["chi"][:, 0:33]
    valid = (c.SC_D_mask[0] != 0)
    m2pi = c.chi_2pi_periodic_mask[0].bool() & valid
    assert int(m2pi.sum()) > 20
    # decoy 1 = decoy 0 + pi on the 2pi-periodic entries: S and C cancel up to the rounding of x + pi in fp32 (half an ulp at 2 pi,
    # 2.4e-7, plus the error of (float)pi, 8.7e-8), so the resultant there is at most about 1.7e-7
    chi1 = torch.where(m2pi, chi0[0] + float(np.pi), chi0[0]).unsqueeze(0)
    chi = torch.cat([chi0, chi1], 1).contiguous()
    r = ctx.ensemble_reduce(chi, 2, per_res=ctx.clash(chi), select="medoid")
    for k in ("mean", "resultant", "dev", "clash", "chi_best"):
        assert torch.isfinite(r[k]).all(), k
    print("cancelled: max resultant", float(r.resultant[0][m2pi].max()))
    assert float(r.resultant[0][m2pi].max()) <= 1e-6
    assert float((r.resultant[0][valid & ~m2pi] - 1).abs().max()) <= 1e-6
    assert r.best.tolist()[0] in (0, 1)
    # two identical decoys: equal scores, the tie goes to index 0 under either rule
    same = torch.cat([chi0, chi0], 1).contiguous()
    pr = ctx.clash(same)
    assert torch.equal(pr[0, :33], pr[0, 33:])
    for sel in ("clash", "medoid"):
        r = ctx.ensemble_reduce(same, 2, per_res=pr, select=sel)
        assert float(r.dev[0]) == float(r.dev[1]) and float(r.clash[0]) == float(r.clash[1])
        assert r.best.tolist() == [0] and torch.equal(r.chi_best, chi0)
    # a NaN score loses to any number: decoy 0's per_res poisoned, decoy 1 wins the clash selection
    bad = pr.clone()
    bad[0, 5] = float("nan")
    r = ctx.ensemble_reduce(same, 2, per_res=bad, select="clash")
    assert bool(torch.isnan(r.clash[0])) and r.best.tolist() == [1]


# ---- 4. invariance ---------------------------------------------------------------------------------------------------------------
def test_a_group_alone_and_packed(model, complexes, two_groups):
    """The L33 group's outputs alone in a context, first in the packed batch, and packed BEHIND the L40 group; and two runs."""
    from packppi_amd.batch import replicate, replicate_many
    t = two_groups
    chi33, chi40 = t["chi"][:, :165].contiguous(), t["chi"][:, 165:].contiguous()
    alone_ctx = _ctx(model, replicate(complexes[0], D))
    behind_ctx = _ctx(model, replicate_many([complexes[1], complexes[0]], D))
    chi_rev = torch.cat([chi40, chi33], 1).contiguous()
    for sel in ("clash", "medoid"):
        first = t[sel]
        alone = alone_ctx.ensemble_reduce(chi33, D, per_res=alone_ctx.clash(chi33), select=sel)
        behind = behind_ctx.ensemble_reduce(chi_rev, D, per_res=behind_ctx.clash(chi_rev), select=sel)
        for k in ("mean", "resultant", "chi_best"):
            assert torch.equal(alone[k][0], first[k][0, :33]) and torch.equal(alone[k][0], behind[k][0, 40:]), (sel, k)
        for k in ("dev", "clash"):
            assert torch.equal(alone[k], first[k][:D]) and torch.equal(alone[k], behind[k][D:]), (sel, k)
        assert alone.best.tolist() == first.best.tolist()[:1] == behind.best.tolist()[1:]
        again = t["ctx"].ensemble_reduce(t["chi"], D, per_res=t["per_res"], select=sel)
        for k in ("mean", "resultant", "dev", "clash", "best", "chi_best"):
            assert torch.equal(again[k], first[k]), (sel, k)


# ---- 5. proximal and selection end to end -----------------------------------------------------------------------------------------
def test_proximal_and_selection(model, complexes):
    from packppi_amd.batch import decoy_key, unpack
    c = complexes[1]
    cfg = model.hparams.sample_cfg
    old = cfg.num_steps
    cfg.num_steps = 5
    try:
        out = model.sample_ensemble(c, 3, seed=SEED, use_proximal=True, select="clash", return_all=True)
        chi, pb = out["decoys"]
        parts = unpack(pb, chi)
        plain = unpack(pb, model.sampling(pb, seed=SEED))
        print("decoys the proximal stage moved:", sum(not torch.equal(a, b) for a, b in zip(parts, plain)), "of 3")
        for d in range(3):
            alone = model.sampling(_solo(c, decoy_key(KEYS[1], d)), use_proximal=True, seed=SEED)
            assert torch.equal(parts[d], alone), d
        clash = out["clash"].cpu().numpy()
        best = int(np.argmin(clash))
        print("proximal ensemble: clash", clash, "best", best)
        assert np.isfinite(clash).all() and out["best"].tolist() == [best] and torch.equal(out["selected"], parts[best])
        assert out["consensus"].shape == (1, 40, 4) and out["confidence"].shape == (1, 40, 4) and out["dev"].shape == (3,)
        assert torch.equal(model.sample_ensemble(c, 3, seed=SEED, use_proximal=True), parts[best])
    finally:
        cfg.num_steps = old


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------------
def _raw(ctx, chi, n_dec, per_res, select, n_cons, n_seg, n_groups):
    """pp_ensemble_reduce itself, past the binding's checks: (status, mean, dev, best, chi_best)."""
    from packppi_amd import lib as L
    f32 = dict(dtype=torch.float32, device=DEV)
    mean, res, best_rows = torch.zeros(n_cons, 4, **f32), torch.zeros(n_cons, 4, **f32), torch.full((n_cons, 4), -7.0, **f32)
    dev, clash = torch.zeros(n_seg, dtype=torch.float64, device=DEV), torch.zeros(n_seg, dtype=torch.float64, device=DEV)
    best = torch.full((max(n_groups, 1),), -9, dtype=torch.int32, device=DEV)
    st = L.load().pp_ensemble_reduce(ctx.handle, L._ptr(chi), n_dec, L._ptr(per_res), select, L._ptr(mean), L._ptr(res), L._ptr(dev),
                                     L._ptr(clash), L._ptr(best), L._ptr(best_rows), L._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return st, mean, dev, best, best_rows


def test_refusals(model, complexes, two_groups):
    from packppi_amd.batch import collate, pack, replicate
    from packppi_amd import lib as L
    c33, c40 = complexes
    ctx = _ctx(model, replicate(c33, 3))
    chi = two_groups["chi"][:, :99].contiguous()
    pr = ctx.clash(chi)
    with pytest.raises(ValueError, match="groups of 2"):                      # n_decoys does not divide B
        ctx.ensemble_reduce(chi, 2, per_res=pr)
    with pytest.raises(ValueError, match="n_decoys"):
        ctx.ensemble_reduce(chi, 0, per_res=pr)
    with pytest.raises(ValueError, match="needs per_res"):                    # select == 1 without per_res
        ctx.ensemble_reduce(chi, 3, select="clash")
    with pytest.raises(ValueError, match="select"):
        ctx.ensemble_reduce(chi, 3, per_res=pr, select="lowest")
    # a hand-made context whose group has unequal lengths: refused from the host table, before any launch
    mixed = _ctx(model, pack([c40, c40, c33, c40, c40, c33]))
    chim = torch.cat([two_groups["chi"][:, a:b] for a, b in ((165, 245), (0, 33), (165, 245), (0, 33))], 1).contiguous()
    with pytest.raises(ValueError, match="differ in length"):
        mixed.ensemble_reduce(chim, 2)
    padded = collate([type(c)({k: (v[0] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}, num_nodes=c.max_size)
                      for c in (c33, c33)])
    with pytest.raises(ValueError, match="padded"):
        _ctx(model, padded).ensemble_reduce(torch.zeros(2, 33, 4, device=DEV), 2)
    # the C entry says PP_ERR_INVALID to the same requests
    for n_dec, per_res, sel in ((2, pr, 0), (0, pr, 0), (3, None, 1), (3, pr, 3)):
        st = _raw(ctx, chi, n_dec, per_res, sel, 99, 3, 1)[0]
        assert st == 1 and b"pp_ensemble_reduce" in L.load().pp_last_error(), (n_dec, sel)
    # ... and past the binding the clamped table keeps a broken group inside the batch: best = -1, dev NaN, its chi_best rows are
    # not written; the intact group in front of it is reduced as usual
    st, mean, dev, best, rows = _raw(mixed, chim, 2, None, 0, 113, 6, 3)
    assert st == 0 and best.tolist() == [0, -1, -1]
    assert torch.isfinite(dev[:2]).all() and torch.isnan(dev[2:]).all()
    assert torch.equal(rows[:40], chim[0, :40]) and bool((rows[40:] == -7).all()) and bool((mean[40:] == 0).all())


# ---- 7. the command line -----------------------------------------------------------------------------------------------------------
def test_cli(tmp_path, capsys):
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion
    from packppi_amd.pdb_io import from_pdb_file, to_pdb
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    out = tmp_path / "out"
    eval_diffusion.main(["--input", str(pdb), "--outdir", str(out), "--molprobity_clash_loc", "/nonexistent", "--device", "cuda",
                         "--random_weights", "3", "--steps", "4", "--n_decoys", "2", "--seed", "3"])
    text = capsys.readouterr().out
    assert "2 decoys in one packed pass" in text and "----- Finishing evaluation! -----" in text
    for name in ("decoy_000.pdb", "decoy_001.pdb", "structure.pdb", "ensemble.csv", "confidence.csv"):
        assert (out / name).exists(), name
    assert not (out / "decoy_002.pdb").exists()
    rows = [ln.split(",") for ln in (out / "ensemble.csv").read_text().splitlines()]
    assert rows[0] == ["decoy", "key", "dev", "clash", "selected"] and [r[0] for r in rows[1:]] == ["0", "1"]
    assert rows[1][1] == "0" and [r[4] for r in rows[1:]].count("1") == 1
    clash = [float(r[3]) for r in rows[1:]]
    best = [r[4] for r in rows[1:]].index("1")
    assert best == int(np.argmin(clash))
    assert (out / "structure.pdb").read_bytes() == (out / f"decoy_{best:03d}.pdb").read_bytes()
    assert (out / "decoy_000.pdb").read_bytes() != (out / "decoy_001.pdb").read_bytes()
    conf = (out / "confidence.csv").read_text().splitlines()
    prot = from_pdb_file(pdb)
    assert conf[0].startswith("chain,residue_number,residue_name,resultant_chi1") and len(conf) == 1 + len(prot["aaindex"])
    first = conf[1].split(",")
    assert first[0] == str(prot["chain_id"][0]) and int(first[1]) == int(prot["residue_index"][0]) and len(first) == 7
    assert all(0.0 <= float(v) <= 1.000001 for ln in conf[1:] for v in ln.split(",")[3:])
