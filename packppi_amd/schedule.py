"""The training-side pieces of the reference's ``SO2Schedule`` (src/models/components/schedule.py:30-94) without its tables.

``so2_score``         SO2Schedule.score(x, sigma): the entry of the 5001 x 5001 table is computed on the device (lib.so2_score).
``score_norm_tables`` SO2Schedule.score_norm_ of the 1pi and the 2pi schedule.

``score_norm_`` is a Monte-Carlo estimate from UNSEEDED ``np.random`` (schedule.py:23-26, 57-63): 10000 draws per grid sigma,
so every entry carries about 1.4 % of sampling noise and the reference's loss differs between processes by about a percent.
``score_norm_tables(seed)`` makes the reference's draws in the reference's order, so a seed gives the table it gives the
reference (up to the few samples per column whose fp32 log lands on the other side of a rounding boundary); every consumer
also takes a table from the caller (``np.save`` of ``np.stack([m.schedule_1pi_periodic.score_norm_,
m.schedule_2pi_periodic.score_norm_])`` from a reference run).
"""
import numpy as np
import torch

from .lib import SO2_GRID, so2_grids, so2_score  # noqa: F401

N_DRAWS = 10000


def score_norm_tables(seed=None, device="cuda", rows_per_launch=500) -> np.ndarray:
    """-> float64 [2, 5001] (1pi schedule, then 2pi).  ``seed``: ``np.random.seed(seed)`` first; None keeps the global stream
    as it is (the reference's behaviour).  Needs about 1 GB of host memory for the 10000 x 5001 draws of one schedule."""
    if seed is not None:
        np.random.seed(seed)
    device = torch.device(device)
    _, sigma_grids = so2_grids()
    out = []
    for pi_periodic, PI, sigma in ((True, 1 / 2 * np.pi, sigma_grids[0]), (False, np.pi, sigma_grids[1])):
        sig = sigma[None].repeat(N_DRAWS, 0).flatten()                       # schedule.py:58-60
        x = sig * np.random.randn(*sig.shape)                                # sample(): one draw of 10000 * 5001
        x = ((x + PI) % (2 * PI) - PI).reshape(N_DRAWS, SO2_GRID)
        sig_dev = torch.from_numpy(sigma).to(device)
        acc = torch.zeros(SO2_GRID, dtype=torch.float64, device=device)
        for r in range(0, N_DRAWS, rows_per_launch):
            xs = torch.from_numpy(x[r:r + rows_per_launch]).to(device)
            s = so2_score(xs, sig_dev[None], pi_periodic)
            acc += (s.double() ** 2).sum(0)
        out.append((acc / N_DRAWS).cpu().numpy())
    return np.stack(out)


def load_score_norm(tables) -> np.ndarray:
    """A caller's table: an ``.npy`` path or an array-like [2, 5001] -> float64 array, validated."""
    if isinstance(tables, torch.Tensor):
        tables = tables.detach().cpu().numpy()
    arr = np.load(tables) if isinstance(tables, (str, bytes)) or hasattr(tables, "__fspath__") else tables
    arr = np.asarray(arr, dtype=np.float64)
    if arr.shape != (2, SO2_GRID) or not np.isfinite(arr).all() or (arr < 0).any():
        raise ValueError(f"score_norm tables must be [2, {SO2_GRID}] finite non-negative numbers (1pi schedule, then 2pi), got {arr.shape}")
    return arr


# ---- clash-guided sampling --------------------------------------------------------------------------------
# Starting values from the CPU oracle on seeded random weights, NOT tuned against a trained checkpoint.
GUIDE_DEFAULTS = dict(scale=0.02, kind="late", t_on=0.3, cap=0.1)
GUIDE_KINDS = ("late", "constant")


def guide_eta(schedule, scale, kind="late", t_on=0.3) -> np.ndarray:
    """The nudge step sizes of ``Context.sample_guided``: float32 [n_schedule], entry j the step size at nudge point j, which sits
    at time ``schedule[j]`` (entry n = n_schedule - 1 belongs to ``schedule[n]``, behind the last reverse step).
    ``kind`` "constant": every entry is ``scale``; "late": ``scale`` where ``schedule[j] <= t_on``, else 0 (no nudge while the
    angles are still mostly noise).  ``scale`` may also be an explicit sequence of n_schedule step sizes, which is passed through
    after validation.  ``ValueError``: a negative or non-finite entry, a wrong length, an unknown kind."""
    sched = np.asarray(torch.as_tensor(schedule, dtype=torch.float32).cpu().numpy(), dtype=np.float32).reshape(-1)
    if sched.size < 2:
        raise ValueError("schedule needs at least 2 times")
    if not np.isscalar(scale) and not (isinstance(scale, (torch.Tensor, np.ndarray)) and np.ndim(scale) == 0):
        eta = np.asarray(torch.as_tensor(scale, dtype=torch.float32).cpu().numpy(), dtype=np.float32).reshape(-1)
        if eta.size != sched.size:
            raise ValueError(f"eta has {eta.size} entries for the {sched.size} nudge points of a schedule of {sched.size} times")
    else:
        scale = float(scale)
        if kind == "constant":
            eta = np.full(sched.size, scale, dtype=np.float32)
        elif kind == "late":
            if not np.isfinite(float(t_on)):
                raise ValueError(f"t_on must be finite, got {t_on!r}")
            eta = np.where(sched <= np.float32(t_on), np.float32(scale), np.float32(0)).astype(np.float32)
        else:
            raise ValueError(f"kind must be one of {list(GUIDE_KINDS)}, got {kind!r}")
    if not np.isfinite(eta).all() or (eta < 0).any():
        raise ValueError("eta entries must be finite and not negative")
    return np.ascontiguousarray(eta, dtype=np.float32)


def resolve_guide(guide, schedule):
    """``guide`` as ``TDiffusionModule.sampling`` takes it -> (eta float32 [n_schedule], cap): a number is the scale of the
    default preset, a dict holds any of ``scale``, ``kind``, ``t_on``, ``cap`` (or ``eta``, an explicit sequence), anything else is
    an explicit eta sequence."""
    cfg = dict(GUIDE_DEFAULTS)
    if isinstance(guide, dict):
        unknown = sorted(set(guide) - set(cfg) - {"eta"})
        if unknown:
            raise ValueError(f"guide has unknown keys {unknown}; known: {sorted(cfg) + ['eta']}")
        cfg.update({k: v for k, v in guide.items() if k != "eta"})
        scale = guide["eta"] if "eta" in guide else cfg["scale"]
    elif isinstance(guide, bool):
        raise ValueError("guide must be a scale, a dict or an eta sequence, not a bool")
    else:
        scale = guide
    cap = float(cfg["cap"])
    if not cap > 0:
        raise ValueError(f"guide cap must be positive (inf = no clamp), got {cfg['cap']!r}")
    return guide_eta(schedule, scale, cfg["kind"], cfg["t_on"]), cap
