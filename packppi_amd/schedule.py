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


# ---- predictor-corrector sampling -------------------------------------------------------------------------
# snr 0.16 is the constant of the reference's SO2VESchedule.step_correct (schedule.py:238), NOT tuned against a trained checkpoint.
CORRECTOR_DEFAULTS = dict(snr=0.16, t_on=1.0, last=False)


def _snr_array(snr, n):
    arr = np.asarray(torch.as_tensor(snr, dtype=torch.float32).cpu().numpy(), dtype=np.float32).reshape(-1)
    if arr.size != n:
        raise ValueError(f"snr has {arr.size} entries for the {n} reverse steps of a schedule of {n + 1} times")
    if not np.isfinite(arr).all() or (arr < 0).any():
        raise ValueError("snr entries must be finite and not negative")
    return np.ascontiguousarray(arr, dtype=np.float32)


def corrector_snr(schedule, snr=0.16, t_on=1.0, last=False) -> np.ndarray:
    """The corrector points of ``Context.sample_corrected``: float32 [n_schedule - 1], entry j the signal-to-noise ratio of the
    Langevin corrector behind reverse step j, which runs at time ``schedule[j + 1]``; 0 = none.  The entry is ``snr`` where
    ``schedule[j + 1] <= t_on``; the one behind the last reverse step is 0 unless ``last`` (a corrector there adds noise to the
    final sample).  ``ValueError``: ``snr`` negative or not finite, ``t_on`` not finite, a schedule of fewer than 2 times."""
    sched = np.asarray(torch.as_tensor(schedule, dtype=torch.float32).cpu().numpy(), dtype=np.float32).reshape(-1)
    if sched.size < 2:
        raise ValueError("schedule needs at least 2 times")
    snr = float(snr)
    if not np.isfinite(snr) or snr < 0:
        raise ValueError(f"snr must be finite and not negative, got {snr!r}")
    if not np.isfinite(float(t_on)):
        raise ValueError(f"t_on must be finite, got {t_on!r}")
    out = np.where(sched[1:] <= np.float32(t_on), np.float32(snr), np.float32(0)).astype(np.float32)
    if not last:
        out[-1] = 0
    return np.ascontiguousarray(out, dtype=np.float32)


def resolve_corrector(corrector, schedule) -> np.ndarray:
    """``corrector`` as ``TDiffusionModule.sampling`` takes it -> snr float32 [n_schedule - 1]: a number is the ``snr`` of the
    default preset, a dict holds any of ``snr``, ``t_on``, ``last`` (``snr`` may be an explicit sequence), anything else is an
    explicit sequence of n_schedule - 1 values, passed through after validation."""
    cfg = dict(CORRECTOR_DEFAULTS)
    if isinstance(corrector, dict):
        unknown = sorted(set(corrector) - set(cfg))
        if unknown:
            raise ValueError(f"corrector has unknown keys {unknown}; known: {sorted(cfg)}")
        cfg.update(corrector)
        snr = cfg["snr"]
    elif isinstance(corrector, bool):
        raise ValueError("corrector must be an snr, a dict or an snr sequence, not a bool")
    else:
        snr = corrector
    if not np.isscalar(snr) and not (isinstance(snr, (torch.Tensor, np.ndarray)) and np.ndim(snr) == 0):
        n = int(torch.as_tensor(schedule).numel()) - 1
        if n < 1:
            raise ValueError("schedule needs at least 2 times")
        return _snr_array(snr, n)
    return corrector_snr(schedule, snr, cfg["t_on"], cfg["last"])


@torch.no_grad()
def step_correct(x, x_score, x_batch, x_mask=None, snr=0.16, noise=None):
    """The reference's ``SO2VESchedule.step_correct`` (schedule.py:238-273) restated in torch, for users of its surface: x, x_score
    [num_res, 4]; x_batch the complex of every ENTRY (anything that reshapes to [num_res, 4], as the reference passes it); x_mask
    bool [num_res, 4] or None = every entry; ``noise`` [num_res, 4] replaces the ``torch.randn_like`` draw (tests).  The norms of
    score and noise are taken per complex over the masked entries and AVERAGED OVER THE COMPLEXES OF THE BATCH into one step size
    ``2 (snr |z| / |s|)^2``: a complex's result depends on what it is batched with.  The device path (``Context.sample_corrected``)
    gives every complex its own step size and is packing-invariant; this function is not, and it does not wrap the angles either,
    as the reference does not."""
    x_batch = x_batch.reshape(-1, 4).long()
    mask = torch.ones_like(x_score, dtype=torch.bool) if x_mask is None else x_mask.bool()
    if noise is None:
        noise = torch.randn_like(x_score)
    idx = x_batch[mask]
    n_seg = int(idx.max()) + 1 if idx.numel() else 0

    def seg_norm(v):
        return torch.sqrt(torch.zeros(n_seg, dtype=v.dtype, device=v.device).index_add_(0, idx, (v ** 2)[mask])).mean()

    step_size = (snr * seg_norm(noise) / seg_norm(x_score)) ** 2 * 2
    x_prev = x.clone()
    x_prev += step_size * x_score
    x_prev += ((step_size * 2) ** 0.5) * noise
    x_prev[~mask] = x[~mask]
    return x_prev
