"""Container-only: run the UNMODIFIED reference's denoising score-matching loss (TorsionalDiffusion.py:126-154) with the REAL
``SO2Schedule`` (schedule.py:30-63: two 5001 x 5001 fp64 tables per schedule and the Monte-Carlo ``score_norm_``) and store
golden vectors.

    PYTHONDONTWRITEBYTECODE=1 python tools/oracle/make_golden_dsm.py --cache /some/scratch/dir

``--cache`` is where the reference writes its tables (800 MB; about five minutes and a few GB of RAM the first time).  It is
REQUIRED: the reference's default lies inside its own source tree.  Nothing in it is ever committed.

refshim's ``build_reference_module`` replaces ``SO2Schedule.__init__`` by a light one; this file does not call it.  The module
is built as ``TDiffusionModule(...)`` with only the DEFAULT of ``SO2VESchedule.__init__``'s ``cache_folder`` changed.  What is
recorded comes out of the reference's own calls: wrappers on bound methods keep the tensors that pass through
(``add_sc_noise``, ``network``, ``score_norm``), and a recording view on ``score_`` keeps the index pair of every lookup.  The
draws are replayed from the recorded seed (``torch.rand`` for t, two ``randn`` for the noise) and checked to reproduce
``SC_D_noised`` bit for bit.  The one piece of arithmetic restated here is the table entry's series, evaluated for the probe
entries forwards and backwards: its forward value is checked to BE the table entry, and |forward - reverse| is stored as the
measure of how many digits the entry carries (the 201 terms cancel at large sigma / PI).

NumPy note: fixtures are made under NumPy 2 (promotion of the fp32 log to fp64 in ``score``); the version is recorded.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, "..", ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import refshim  # noqa: E402
from packppi_amd.weights import make_random_state_dict  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
WEIGHT_SEED = 20251003
NP_SEED = 20261016              # np.random.seed before the module is built: score_norm_ of the 1pi, then of the 2pi schedule
PROBE_SEED = 812
N_PROBE = 4096
CASES = {"L64": ("g2_ops_L64", 1201), "B3": ("g2_ops_B3", 1202), "T1124": ("g4_T1124", 1203)}     # fixture of the batch, torch seed


class RecordingTable:
    """``score_[sigma_idx, x_idx]`` with the index pair kept."""

    def __init__(self, table):
        self.table, self.last = table, None

    def __getitem__(self, idx):
        self.last = idx
        return self.table[idx]


def build_module(cache):
    import src.models.components.schedule as sch
    import src.models.TorsionalDiffusion as TD
    d = list(sch.SO2VESchedule.__init__.__defaults__)
    assert d[1] is None
    d[1] = cache                                                    # cache_folder: the default only, no code replaced
    sch.SO2VESchedule.__init__.__defaults__ = tuple(d)
    np.random.seed(NP_SEED)
    torch.manual_seed(0)
    model = TD.TDiffusionModule(optimizer=None, scheduler=None, encoder_cfg=refshim.ENC, model_cfg=refshim.MDL,
                                sample_cfg=refshim.SMP).eval()
    model.load_state_dict(make_random_state_dict(WEIGHT_SEED), strict=True)
    return model


def load_batch(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    d = refshim.Data()
    for k in z.files:
        if k.startswith("batch."):
            key = k[6:]
            d[key] = int(z[k]) if key in ("num_proteins", "max_size") else torch.from_numpy(z[k])
    return d


def series(x, sigma, PI, order):
    p = np.zeros_like(x)
    g = np.zeros_like(x)
    for i in order:
        e = np.exp(-(x + 2 * PI * i) ** 2 / 2 / sigma ** 2)
        p += e
        g += (x + 2 * PI * i) / sigma ** 2 * e
    return g / np.where(p == 0, 1e-10, p)


def probes(sched, rng):
    PI = sched.PI
    sigma = np.exp(rng.uniform(np.log(0.01 * np.pi), np.log(np.pi), N_PROBE - 64)).astype(np.float32)
    x = (sigma * rng.standard_normal(sigma.shape)).astype(np.float32)
    cs = np.array([1e-3, 3e-3, 3.0001e-3, 0.01, 0.1, 1.0, 2.0, 3.0], np.float64) * PI                      # both clip ends and beyond
    cx = np.array([0.0, PI, -PI, np.nextafter(np.float32(PI), np.float32(0)), 1e-6 * PI, 1e-5 * PI, 0.5 * PI, -0.25 * PI])
    gs, gx = np.meshgrid(cs, cx, indexing="ij")
    sigma = np.concatenate([sigma, gs.ravel().astype(np.float32)])
    x = np.concatenate([x, gx.ravel().astype(np.float32)])
    assert x.shape == (N_PROBE,)
    rec = RecordingTable(sched.score_)
    sched.score_ = rec
    try:
        val = sched.score(x, sigma)                          # fp32 arrays, as add_noise hands them over
    finally:
        sched.score_ = rec.table
    si, xi = rec.last
    fwd = series(sched.x[xi], sched.sigma[si], PI, range(-100, 101))
    rev = series(sched.x[xi], sched.sigma[si], PI, range(100, -101, -1))
    same = np.array_equal(fwd, rec.table[si, xi])
    print(f"  PI={PI:.3f}: forward series == table entry on all probes: {same}; max |fwd-rev| {np.abs(fwd - rev).max():.3e}")
    assert (np.abs(fwd - rec.table[si, xi]) <= 4 * np.abs(fwd - rev) + 1e-12 * np.abs(fwd)).all()
    return dict(x=x, sigma=sigma, score=torch.tensor(val, dtype=torch.float32).numpy(), score_f64=val,
                sigma_idx=si.astype(np.int32), x_idx=xi.astype(np.int32), fwd_rev=np.abs(rec.table[si, xi] - rev))


def run_case(model, tag, src, seed):
    b = load_batch(src)
    B, L = b.residue_type.shape
    N = B * L
    kept = {}
    add, net = model.add_sc_noise, model.network
    sn1, sn2 = model.schedule_1pi_periodic.score_norm, model.schedule_2pi_periodic.score_norm

    def keep(name, fn):
        def w(*a, **k):
            out = fn(*a, **k)
            kept[name] = out
            return out
        return w

    model.add_sc_noise, model.network = keep("add", add), keep("net", net)
    model.schedule_1pi_periodic.score_norm, model.schedule_2pi_periodic.score_norm = keep("sn1", sn1), keep("sn2", sn2)
    try:
        torch.manual_seed(seed)
        with torch.no_grad():
            loss = model.forward(b)
    finally:
        del model.add_sc_noise, model.network, model.schedule_1pi_periodic.score_norm, model.schedule_2pi_periodic.score_norm
    # replay the draws of that seed: sample_train_t, then the two randn_like of add_noise
    torch.manual_seed(seed)
    t = torch.rand((B,))
    noise = torch.stack([torch.randn(N, 4), torch.randn(N, 4)])
    noised, target = kept["add"]
    pred = kept["net"][0]
    sig = model.schedule_1pi_periodic.t_to_sigma(t.repeat_interleave(L)).unsqueeze(-1)
    x = b.SC_D.reshape(-1, 4)
    x = x + noise[0] * sig * b.chi_1pi_periodic_mask.reshape(-1, 4)
    x = x + noise[1] * sig * b.chi_2pi_periodic_mask.reshape(-1, 4)
    x = (x + np.pi) % (2 * np.pi) - np.pi
    assert torch.equal(x.reshape(B, L, 4), noised), "replayed draws do not reproduce SC_D_noised"
    sn = torch.where(b.chi_1pi_periodic_mask.reshape(-1, 4), torch.tensor(kept["sn1"]), torch.tensor(kept["sn2"])).reshape(B, L, 4)
    scaled = pred * torch.sqrt(sn) * b.SC_D_mask
    num = ((target - scaled) ** 2 / (sn + model.eps)).sum(dim=(1, 2))
    den = b.SC_D_mask.double().sum(dim=(1, 2))
    chk = num.sum() / (den.sum() if den.sum() > 0 else 1)
    assert abs(chk.item() - loss.item()) <= 1e-12 * abs(loss.item()), (chk, loss)
    print(f"  {tag}: t {t.tolist()} loss {loss.item():.9f} dtype {loss.dtype}")
    out = dict(seed=np.int64(seed), t=t.numpy(), noise=noise.numpy(), SC_D_noised=noised.numpy(), target_score=target.numpy(),
               pred_score=pred.numpy(), score_norm_1pi=np.asarray(kept["sn1"]).reshape(B, L, 4),
               score_norm_2pi=np.asarray(kept["sn2"]).reshape(B, L, 4), loss=np.float64(loss.item()), num=num.numpy(),
               den=den.numpy(), batch_fixture=src)
    path = os.path.join(GOLD, f"g12_dsm_{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote {os.path.basename(path)}  {os.path.getsize(path) / 1e6:.3f} MB")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cache", required=True, help="scratch directory for the reference's tables (never inside the reference tree)")
    ap.add_argument("--threads", type=int, default=8)
    args = ap.parse_args()
    cache = os.path.abspath(os.path.expanduser(args.cache))
    assert not cache.startswith(os.path.abspath(refshim.REF)), "--cache must lie outside the reference tree"
    torch.set_num_threads(args.threads)
    model = build_module(cache)
    s1, s2 = model.schedule_1pi_periodic, model.schedule_2pi_periodic
    rng = np.random.default_rng(PROBE_SEED)
    out = dict(score_norm=np.stack([s1.score_norm_, s2.score_norm_]), np_seed=np.int64(NP_SEED), numpy_version=np.__version__,
               x_grid=np.stack([s1.x, s2.x]), sigma_grid=np.stack([s1.sigma, s2.sigma]))
    for name, s in (("1pi", s1), ("2pi", s2)):
        for k, v in probes(s, rng).items():
            out[f"{name}.{k}"] = v
    path = os.path.join(GOLD, "g12_dsm_tables.npz")
    np.savez_compressed(path, **out)
    print(f"  wrote g12_dsm_tables.npz  {os.path.getsize(path) / 1e6:.3f} MB")
    for tag, (src, seed) in CASES.items():
        run_case(model, tag, src, seed)


if __name__ == "__main__":
    main()
