"""pp_ensemble_recombine on the device (csrc/pp_recombine.hip) against the fp64 restatement of
tests/test_recombine_host.py, on its inputs A (33 rows), B (64), C (97), four decoys each, 64 sweeps, and on dense_complex() of
tests/test_clash_capacity.py, where a row has 306 partners: more than the kernel's partner lists hold, so those rows scan their group.

Bounds (none of them taken from what the device gives; measured values are in profiles/r18_recombine_parity.txt):
  tolE = 1e-4 + 4e-6 |E|  a local energy against fp64: the project's bound for the same arithmetic (per_res within 5e-5 at values up
                          to ~20, tests/test_hip_parity.py), doubled because E carries both residues' weights;
  2e-5                    what two evaluations of one structure's mean clash may differ by (tests/test_hip_parity.py): the slack of the
                          monotonicity check, which the accept-every-proposal rule breaks by 50 times and more on these inputs
                          (test_recombine_host.py::test_accepting_every_proposal_is_not_monotone);
  5e-5                    a mean clash against another evaluation of it by pp_clash (the per_res bound above).
"""
import functools

import numpy as np
import pytest
import torch

from . import test_recombine_host as H

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
VTF, TOL = H.VTF, H.TOL
NAMES = list(H.CASES)
SEED = 0x1234_5678_9abc_def0


def tol_e(E):
    return 1e-4 + 4e-6 * np.abs(E)


def _ctx(batch):
    from packppi_amd.functional import _ctx_for
    return _ctx_for(batch)


def _flat(chis):
    """[D, L, 4] -> the packed ensemble's [1, D L, 4] on the device."""
    return chis.reshape(1, -1, 4).to(DEV).contiguous()


class Dev:
    """A host case on the device: the packed ensemble, its reduction and the 64-sweep recombination from the device's `best`.
    Computed once, shared, never modified."""

    def __init__(self, host, max_sweeps=64):
        from packppi_amd.batch import replicate
        self.h, self.D, self.n = host, host.D, host.n
        self.gb = host.b.to(DEV)
        self.pb = replicate(self.gb, host.D)
        assert self.pb.seg_offsets_host == [d * host.n for d in range(host.D + 1)]
        self.chi = _flat(host.chis)
        self.ctx = _ctx(self.pb)
        self.per_res = self.ctx.clash(self.chi, VTF, TOL)
        self.red = self.ctx.ensemble_reduce(self.chi, host.D, per_res=self.per_res, select="clash")
        self.rec = self.ctx.ensemble_recombine(self.chi, host.D, start=self.red.best, max_sweeps=max_sweeps, want_energy=True)
        self.start = int(self.red.best[0])


@functools.lru_cache(maxsize=None)
def dev(name):
    return Dev(H.case(name))


class DenseCase(H.Case):
    """dense_complex() with two uniform decoys (rng of the named inputs: default_rng(170 + n + 1))."""

    def __init__(self):
        from .test_clash_capacity import DENSE_L, dense_complex
        self.name, self.n, self.D = "dense", DENSE_L, 2
        self.b = dense_complex()
        self.chis = H.decoy_angles(self.b, DENSE_L, 2, "uniform")

    @functools.cached_property
    def run(self):
        return H.descend(*self.UW, self.P, self.best, 384)


@functools.lru_cache(maxsize=None)
def dense():
    """The ball's 307 rows are pairwise partners, so a sweep moves one of them: the restatement needs 156 sweeps.  The cap is 384,
    the same 2.5 times what the restatement needs that 64 sweeps are for input C (26)."""
    return Dev(DenseCase(), max_sweeps=384)


def check_arithmetic(d):
    U, W = d.h.UW
    want = H.local_energy(U, W, np.full(d.n, d.start))
    got = d.rec.energy.cpu().double().numpy()
    err = np.abs(got - want)
    print(f"{d.h.name}: max |E device - E fp64| {err.max():.2e} at |E| up to {np.abs(want).max():.1f} (bound 1e-4 + 4e-6 |E|), "
          f"worst ratio to the bound {(err / tol_e(want)).max():.3f}")
    assert d.start == d.h.best
    assert (err <= tol_e(want)).all()


def check_is_a_recombination(d, rec=None):
    rec = rec or d.rec
    pick = rec.pick.long()
    assert bool(((pick >= 0) & (pick < d.D)).all())
    rows = pick * d.n + torch.arange(d.n, device=DEV)
    assert torch.equal(rec.chi[0], d.chi[0, rows])


def check_descent(d):
    from packppi_amd.batch import replicate
    trace = d.rec.clash_trace[0].cpu().numpy()
    ref = d.h.run[1]
    print(f"{d.h.name}: device trace {trace[0]:.6f} -> {trace[-1]:.6f} in {int(d.rec.sweeps[0])} sweeps, "
          f"{int((d.rec.pick != d.start).sum())} rows moved; fp64 {ref[0]:.6f} -> {ref[-1]:.6f}; "
          f"largest rise in one sweep {np.diff(trace).max():.2e}")
    assert int(d.rec.converged[0]) == 1
    assert (np.diff(trace) <= 2e-5).all()
    assert abs(trace[0] - float(d.red.clash[d.start])) <= 5e-5
    one = _ctx(replicate(d.gb, 1))
    final = float(one.clash(d.rec.chi, VTF, TOL).double().mean())
    assert abs(trace[-1] - final) <= 5e-5, (trace[-1], final)
    assert trace[0] - trace[-1] >= 0.5 * (ref[0] - ref[-1])


def check_local_optimum(d):
    U, W = d.h.UW
    pick = d.rec.pick.cpu().numpy()
    E = H.local_energy(U, W, pick)
    mine = E[np.arange(d.n), pick]
    assert (mine <= E.min(1) + 2 * tol_e(mine)).all(), float((mine - E.min(1)).max())


# ---- 1 - 4 on A, B, C ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_local_energies_against_fp64(name):
    check_arithmetic(dev(name))


@pytest.mark.parametrize("name", NAMES)
def test_result_is_a_recombination(name):
    check_is_a_recombination(dev(name))


@pytest.mark.parametrize("name", NAMES)
def test_descent(name):
    check_descent(dev(name))


@pytest.mark.parametrize("name", NAMES)
def test_final_assignment_is_a_local_optimum(name):
    check_local_optimum(dev(name))


# ---- 5. no gratuitous moves --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_rows_without_an_angle_keep_the_start(name):
    d = dev(name)
    still = (d.gb.SC_D_mask[0] == 0).all(-1)
    assert still.any() and bool((d.rec.pick[still] == d.start).all())


def test_identical_decoys_one_decoy_and_few_sweeps():
    from packppi_amd.batch import replicate
    d = dev("B")
    same = d.chi[:, :d.n].repeat(1, d.D, 1).contiguous()
    start = torch.tensor([2], dtype=torch.int32, device=DEV)
    r = d.ctx.ensemble_recombine(same, d.D, start=start)
    assert bool((r.pick == 2).all()) and int(r.sweeps[0]) == 0 and int(r.converged[0]) == 1
    assert torch.equal(r.chi, same[:, :d.n]) and bool((r.clash_trace[0] == r.clash_trace[0, 0]).all())
    # one decoy: nothing to choose
    one = _ctx(replicate(d.gb, 1))
    for k in (0, 3):
        r = one.ensemble_recombine(d.chi[:, :d.n].contiguous(), 1, max_sweeps=k)
        assert torch.equal(r.chi, d.chi[:, :d.n]) and int(r.converged[0]) == 1 and int(r.sweeps[0]) == 0 and not r.pick.any()
    # no sweep: the start decoy's rows, not converged; start = None is decoy 0
    r = d.ctx.ensemble_recombine(d.chi, d.D, start=d.red.best, max_sweeps=0)
    assert torch.equal(r.chi, d.red.chi_best) and int(r.converged[0]) == 0 and r.clash_trace.shape == (1, 1)
    assert torch.equal(r.clash_trace[0, 0], d.rec.clash_trace[0, 0])
    r = d.ctx.ensemble_recombine(d.chi, d.D, max_sweeps=0)
    assert torch.equal(r.chi, d.chi[:, :d.n]) and not r.pick.any()
    # one sweep
    r = d.ctx.ensemble_recombine(d.chi, d.D, start=d.red.best, max_sweeps=1)
    t = r.clash_trace[0].cpu().numpy()
    assert t[1] <= t[0] and int((r.pick != d.start).sum()) >= 1 and int(r.sweeps[0]) == 1
    assert torch.equal(r.clash_trace[0], d.rec.clash_trace[0, :2])
    check_is_a_recombination(d, r)


# ---- 6. placement ------------------------------------------------------------------------------------------------------------------------
def test_a_group_alone_and_packed_and_twice():
    from packppi_amd.batch import replicate_many
    a, b = dev("A"), dev("B")
    again = a.ctx.ensemble_recombine(a.chi, a.D, start=a.red.best, max_sweeps=64, want_energy=True)
    for k in ("pick", "chi", "clash_trace", "sweeps", "converged", "energy"):
        assert torch.equal(again[k], a.rec[k]), k
    for order in ((a, b), (b, a)):
        pb = replicate_many([x.gb for x in order], 4)
        chi = torch.cat([x.chi for x in order], 1).contiguous()
        ctx = _ctx(pb)
        start = torch.cat([x.red.best for x in order])
        r = ctx.ensemble_recombine(chi, 4, start=start, max_sweeps=64, want_energy=True)
        g = order.index(a)
        lo = 0 if g == 0 else b.n
        assert torch.equal(r.pick[lo:lo + a.n], a.rec.pick) and torch.equal(r.chi[:, lo:lo + a.n], a.rec.chi)
        assert torch.equal(r.clash_trace[g], a.rec.clash_trace[0]) and torch.equal(r.sweeps[g:g + 1], a.rec.sweeps)
        assert torch.equal(r.energy[lo:lo + a.n], a.rec.energy) and torch.equal(r.converged[g:g + 1], a.rec.converged)
        assert torch.equal(r.clash_trace[1 - g], b.rec.clash_trace[0])


# ---- 7. more partners than the lists hold ---------------------------------------------------------------------------------------------------
def test_rows_with_more_partners_than_the_lists_hold():
    from .test_clash_capacity import CAP
    d = dense()
    n_partners = d.h.P.sum(1)
    assert n_partners.max() > 2 * CAP and (n_partners == 0).any()          # rows that scan their group, rows with an empty list
    check_arithmetic(d)
    check_is_a_recombination(d)
    check_descent(d)
    check_local_optimum(d)


# ---- 8. refusals -------------------------------------------------------------------------------------------------------------------------
def _raw(ctx, chi, n_dec, start, max_sweeps, n_cons, n_groups, null=None):
    """pp_ensemble_recombine itself, past the binding's checks: (status, pick, chi_out, trace, sweeps, converged)."""
    from packppi_amd import lib as L
    pick = torch.full((n_cons,), -9, dtype=torch.int32, device=DEV)
    out = torch.full((n_cons, 4), -7.0, device=DEV)
    trace = torch.full((max(n_groups, 1), max(max_sweeps, 0) + 1), -5.0, dtype=torch.float64, device=DEV)
    sweeps = torch.full((max(n_groups, 1),), -3, dtype=torch.int32, device=DEV)
    conv = torch.full((max(n_groups, 1),), -3, dtype=torch.int32, device=DEV)
    args = dict(chi=chi, pick=pick, chi_out=out, trace=trace, sweeps=sweeps, converged=conv)
    if null:
        args[null] = None
    st = L.load().pp_ensemble_recombine(ctx.handle if null != "ctx" else None, L._ptr(args["chi"]), n_dec, L._ptr(start), max_sweeps,
                                        L._ptr(args["pick"]), L._ptr(args["chi_out"]), L._ptr(args["trace"]), L._ptr(args["sweeps"]),
                                        L._ptr(args["converged"]), None, L._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    return st, pick, out, trace, sweeps, conv


def test_refusals():
    from packppi_amd import lib as L
    from packppi_amd.batch import Batch, collate, pack, replicate
    a, b, c = dev("A"), dev("B"), dev("C")
    err = lambda: L.load().pp_last_error()
    with pytest.raises(ValueError, match="groups of 3"):
        a.ctx.ensemble_recombine(a.chi, 3)
    with pytest.raises(ValueError, match="n_decoys"):
        a.ctx.ensemble_recombine(a.chi, 0)
    with pytest.raises(ValueError, match="max_sweeps"):
        a.ctx.ensemble_recombine(a.chi, 4, max_sweeps=-1)
    with pytest.raises(ValueError, match="start has"):
        a.ctx.ensemble_recombine(a.chi, 4, start=torch.zeros(2, dtype=torch.int32))
    for null in ("ctx", "chi", "pick", "chi_out", "trace", "sweeps", "converged"):
        assert _raw(a.ctx, a.chi, 4, None, 2, a.n, 1, null=null)[0] == 1 and b"pp_ensemble_recombine" in err(), null
    for n_dec, sweeps in ((0, 2), (3, 2), (4, -1)):
        assert _raw(a.ctx, a.chi, n_dec, None, sweeps, a.n, 1)[0] == 1 and b"pp_ensemble_recombine" in err(), (n_dec, sweeps)
    single = lambda c: Batch({k: (v[0] if isinstance(v, torch.Tensor) else v) for k, v in c.items()}, num_nodes=c.max_size)
    padded = _ctx(collate([single(a.gb), single(a.gb)]))
    with pytest.raises(ValueError, match="padded"):
        padded.ensemble_recombine(torch.zeros(2, a.n, 4, device=DEV), 2)
    assert _raw(padded, torch.zeros(2, a.n, 4, device=DEV), 2, None, 2, a.n, 1)[0] == 1 and b"padded" in err()
    bare = _ctx(Batch({k: v for k, v in a.pb.items() if k not in ("atom_mask", "residue_index")}))
    assert _raw(bare, a.chi, 4, None, 2, a.n, 1)[0] == 1 and b"atom_mask / residue_index" in err()
    # a start outside 0 .. D - 1: the group is left alone, the group next to it is recombined as usual
    from packppi_amd.batch import replicate_many
    pb = replicate_many([a.gb, b.gb], 4)
    chi = torch.cat([a.chi, b.chi], 1).contiguous()
    ctx = _ctx(pb)
    for bad in (-1, 4):
        start = torch.tensor([bad, int(b.red.best[0])], dtype=torch.int32, device=DEV)
        st, pick, out, trace, sweeps, conv = _raw(ctx, chi, 4, start, 64, a.n + b.n, 2)
        assert st == 0 and bool((pick[:a.n] == -1).all()) and bool((out[:a.n] == -7).all()) and bool(torch.isnan(trace[0]).all())
        assert sweeps.tolist() == [0, int(b.rec.sweeps[0])] and conv.tolist() == [0, 1]
        assert torch.equal(pick[a.n:], b.rec.pick) and torch.equal(out[a.n:], b.rec.chi[0]) and torch.equal(trace[1], b.rec.clash_trace[0])
    # a group of unequal lengths: refused from the host table; past the binding it is left alone, inside the batch
    mixed = _ctx(pack([b.gb, b.gb, a.gb, c.gb]))
    chim = torch.cat([b.chi[:, :2 * b.n], a.chi[:, :a.n], c.chi[:, :c.n]], 1).contiguous()
    with pytest.raises(ValueError, match="differ in length"):
        mixed.ensemble_recombine(chim, 2)
    n_cons = (2 * b.n + a.n + c.n) // 2
    st, pick, out, trace, sweeps, conv = _raw(mixed, chim, 2, None, 8, n_cons, 2)
    assert st == 0 and bool((pick[:b.n] >= 0).all()) and bool((pick[b.n:] == -1).all()) and bool((out[b.n:] == -7).all())
    assert bool(torch.isfinite(trace[0]).all()) and bool(torch.isnan(trace[1]).all()) and sweeps[1] == 0 and conv[1] == 0


# ---- 9. surfaces ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(weights):
    from packppi_amd.module import TDiffusionModule
    m = TDiffusionModule(weights, device=DEV)
    m.schedule = torch.linspace(1, 0, 11)
    return m


@pytest.fixture(scope="module")
def c64():
    from packppi_amd import synth
    from packppi_amd.featurize import protein_to_batch
    c = protein_to_batch(synth.make_complex(64, 70 + 64)).to(DEV)
    c["complex_key"], c["complex_keys"] = 7, [7]
    return c


def _check_rows(out, D, n):
    chi, _ = out["decoys"]
    pick = out["pick"].long()
    assert bool(((pick >= 0) & (pick < D)).all())
    assert torch.equal(out["recombined"][0], chi[0, pick * n + torch.arange(n, device=DEV)])
    t = out["clash_trace"][0]
    assert float(t[-1]) <= float(t[0]) + 2e-5 and abs(float(t[0]) - float(out["clash"][int(out["best"][0])])) <= 5e-5


def test_sample_ensemble(model, c64):
    plain = model.sample_ensemble(c64, 4, seed=SEED, return_all=True)
    out = model.sample_ensemble(c64, 4, seed=SEED, return_all=True, recombine=True)
    assert set(out) - set(plain) == {"recombined", "pick", "clash_trace", "sweeps", "converged"}
    for k in ("selected", "best", "dev", "clash", "consensus", "confidence"):
        assert torch.equal(out[k], plain[k]), k
    assert torch.equal(out["decoys"][0], plain["decoys"][0])
    _check_rows(out, 4, 64)
    assert out["clash_trace"].shape == (1, 65)
    assert torch.equal(model.sample_ensemble(c64, 4, seed=SEED, recombine=True), out["recombined"])
    assert torch.equal(model.sample_ensemble(c64, 4, seed=SEED), plain["selected"])
    few = model.sample_ensemble(c64, 4, seed=SEED, return_all=True, recombine=True, recombine_sweeps=2, select=None)
    assert few["clash_trace"].shape == (1, 3) and int(few["best"][0]) == 0
    _check_rows(few, 4, 64)


def test_repack_ensemble_keeps_the_fixed_rows(model, c64):
    fixed = (torch.arange(64, device=DEV) % 3 != 0).reshape(1, 64)
    old = model.hparams.sample_cfg.num_steps
    for use_proximal in (False, True):
        model.hparams.sample_cfg.num_steps = 5
        try:
            out = model.repack_ensemble(c64, fixed, n_decoys=4, seed=SEED, use_proximal=use_proximal, return_all=True, recombine=True)
        finally:
            model.hparams.sample_cfg.num_steps = old
        _check_rows(out, 4, 64)
        assert torch.equal(out["recombined"][fixed], c64.SC_D[fixed])
        assert bool((out["pick"][fixed[0]] == out["best"][0]).all())


def test_mutate(model):
    from .test_mutate_host import protein_1brs
    p = protein_1brs()
    quiet = dict(seed=SEED, n_decoys=3, log=lambda s: None)
    plain = model.mutate([(p, "LA87F")], **quiet)[0]
    alone = model.mutate([(p, "LA87F")], recombine=True, **quiet)[0]
    both = model.mutate([(p, "SA89A,DD39A", 5), (p, "LA87F", 0)], recombine=True, **quiet)[1]
    assert set(alone) - set(plain) == {"pick", "clash_recombined", "rows_recombined"}
    for k in ("shell", "best", "clash", "dev"):
        assert torch.equal(alone[k], plain[k]), k
    for k in ("SC_D", "X", "pick", "clash_recombined", "rows_recombined", "shell", "best"):
        assert torch.equal(both[k], alone[k]), k
    outside = ~alone["shell"]
    wt = alone["batch"].SC_D
    assert torch.equal(alone["SC_D"][outside], wt[outside]) and bool((alone["pick"][outside] == alone["best"]).all())
    assert alone["pick"].shape == (1, 195) and int(alone["rows_recombined"]) == int((alone["pick"] != alone["best"]).sum())
    assert float(alone["clash_recombined"]) <= float(alone["clash"][int(alone["best"])]) + 2e-5


def test_command_lines(tmp_path, capsys):
    from packppi_amd import synth
    from packppi_amd.cli import eval_diffusion, mutate
    from packppi_amd.pdb_io import to_pdb
    from .test_mutate_host import protein_1brs
    pdb = tmp_path / "complex.pdb"
    pdb.write_text(to_pdb(synth.make_complex(60, 21)))
    base = ["--input", str(pdb), "--molprobity_clash_loc", "/nonexistent", "--device", "cuda", "--random_weights", "3", "--steps", "4",
            "--n_decoys", "3", "--seed", "3"]
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "plain")])
    eval_diffusion.main(base + ["--outdir", str(tmp_path / "rec"), "--recombine", "--recombine_sweeps", "32"])
    assert "recombined per residue" in capsys.readouterr().out
    plain, rec = tmp_path / "plain", tmp_path / "rec"
    same = ["decoy_000.pdb", "decoy_001.pdb", "decoy_002.pdb", "ensemble.csv", "confidence.csv"]
    assert not (plain / "recombined.pdb").exists() and not (plain / "recombine.csv").exists()
    for name in same:
        assert (rec / name).read_bytes() == (plain / name).read_bytes(), name
    assert (rec / "structure.pdb").read_bytes() == (rec / "recombined.pdb").read_bytes()
    rows = [ln.split(",") for ln in (rec / "recombine.csv").read_text().splitlines()]
    assert rows[0] == ["chain", "residue_number", "residue_name", "decoy", "energy_before", "energy_after"] and len(rows) == 61
    best = [r[4] for r in [ln.split(",") for ln in (rec / "ensemble.csv").read_text().splitlines()][1:]].index("1")
    picks = [int(r[3]) for r in rows[1:]]
    assert all(0 <= d < 3 for d in picks) and all(np.isfinite(float(r[4])) and np.isfinite(float(r[5])) for r in rows[1:])
    if any(d != best for d in picks):
        assert (rec / "structure.pdb").read_bytes() != (plain / "structure.pdb").read_bytes()
        assert sum(float(r[5]) for r in rows[1:]) < sum(float(r[4]) for r in rows[1:])
    else:
        assert (rec / "structure.pdb").read_bytes() == (plain / "structure.pdb").read_bytes()
    # mutate
    brs = tmp_path / "1brs.pdb"
    brs.write_text(to_pdb(protein_1brs()))
    mbase = ["--input", str(brs), "--mutstr", "LA87F", "--device", "cuda", "--random_weights", "3", "--steps", "3", "--seed", "7",
             "--n_decoys", "2"]
    mutate.main(mbase + ["--outdir", str(tmp_path / "mplain")])
    mutate.main(mbase + ["--outdir", str(tmp_path / "mrec"), "--recombine"])
    assert "residues recombined from other decoys" in capsys.readouterr().out
    head = lambda d: [ln.split(",") for ln in (tmp_path / d / "mutants.csv").read_text().splitlines()]
    assert head("mplain")[0] == ["tag", "shell_rows", "selected_decoy", "clash", "dev"]
    assert head("mrec")[0] == ["tag", "shell_rows", "selected_decoy", "clash", "dev", "clash_recombined", "rows_recombined"]
    assert head("mrec")[1][:5] == head("mplain")[1] and float(head("mrec")[1][5]) <= float(head("mrec")[1][3]) + 2e-5
    assert (tmp_path / "mrec" / "mutant_LA87F.pdb").exists()
    if int(head("mrec")[1][6]) == 0:
        assert (tmp_path / "mrec" / "mutant_LA87F.pdb").read_bytes() == (tmp_path / "mplain" / "mutant_LA87F.pdb").read_bytes()
